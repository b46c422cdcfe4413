"""Collection on the device: what a training step does around the step kernel, in two calls.

Between ``hkl_explore`` and the next step, ``train`` / ``train_population`` run player 2's opponent draw
(``opponents._draw``, ``torch.multinomial``, the counts), four clones of the step's outputs, ``store_step``, the ragged
``PopulationRing.push``, the outcome tally and -- under ``episode_end="done"`` -- two host syncs as a few dozen small
torch launches.  Every piece is a function of one arena row, a few words per member and a counter-based draw, so two
entry points of the learner library (include/hockey_collect.h, csrc/hkl_collect.h) run them:

* ``hkl_opp_draw`` before the step: bot or self-play, which bot, which snapshot, the bots' phase increments and the
  round's opponent counts, one lane per arena;
* ``hkl_collect`` after it: the replay store in arena order per member with the ring's wrap-around, the write positions
  and fill levels, the episode rewards, the outcome tally, the step counts, the survivors and the copies that keep
  the step's observations.

One ``Collector.step()`` is ``hkl_explore``, ``hkl_opp_draw``, one ``PolicyBank.act`` for the self-play arenas, the
step kernel, ``hkl_collect`` and, with prioritized members, ``hkl_per_push_group``: no torch op on a tensor of N rows
in between, nothing read back.  ``PopulationOpponentMix`` keeps the pools, the wide bank, ``snapshot`` and the
round-end fold; the Collector uploads its scores / slots / lengths and the curriculum row once per round and replaces
only the per-step ``select`` and ``register_outcomes``.

The laws, for member m owning rows [m n, (m + 1) n) and local(i) = i - m n, are stated in include/hockey_collect.h and
restated here in numpy (``opp_draw_law``, ``collect_law``): backend="torch" runs them in place of the kernels, on any
device -- slow, and the executable specification the GPU tests hold the kernels to, word for word.

Draws are Philox4x32-10 blocks keyed by ``seed_m ^ purpose`` at counter (local(i), calls[m]), as the Explorer's: member
j's opponent draws and bot phase increments are the same bits alone and inside a population of 64.  With
``explore="device"`` a member's whole run -- trajectories, ring, weights -- then no longer depends on the population.

Batched differences from the torch path (``collect="torch"``), by design: the draws are Philox's,
keyed per member, not one torch generator's over the population; the opponent counts are taken over the arenas still
running (identical under ``episode_end="max_steps"``); the bots' phase increments are supplied per member
(``hk_step_io.opp_inc``) instead of drawn by the step kernel from the global arena id, and the bots' phases are set
per member from a host draw, at construction and again at every round's start (the torch path lets them walk on
across rounds); the per-member opponent counts are reported also without self-play.

``episode_end="done"``: the host reads the survivors' count every ``poll_every`` steps only.  A step with nobody alive
stores nothing, counts nothing and advances nothing but the call counters of the two draws, and the Explorer's noise
state that it touches is reset at the next round's start; at a round's end the Collector sets both call counters of
member m to their value at the round's start plus the steps in which m still had a running arena (``live``, counted on
the device), so neither ``poll_every`` nor the other members' episodes reach a member's later draws.  An arena whose
episode ended is still stepped until the round ends, and ``HockeyEnv.reset`` keeps the players' has-puck timers (the
reference's does too), so under "done" the Collector clears the arenas' episode words (``set_state(aux=0)``: the timers,
time, done, winner) at a round's end: the next reset then starts from the same state however long the round ran on.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native as N
from .explore import GROUP_MAX
from .philox_ref import U64, draw_words, phase_inc, u24, u53  # noqa: F401 (u53: re-exported)
from .policy_bank import resolve_backend

KEY_OPP = 0x6F70706F6E656E74  # HKL_COLLECT_KEY_OPP ("opponent")
KEY_PHASE = 0x7068617365  # HKL_COLLECT_KEY_PHASE ("phase")
PHASE_TAG = 0x626F7473  # "bots": the host generator of a member's phases in a round is default_rng([seed, PHASE_TAG, round])


# ---------------------------------------------------------------------------------------------------- the laws in numpy
def opp_draw_law(seeds, n, calls, probs, lens, scores, slots, alive=None, counts=None, snap_counts=None):
    """One ``hkl_opp_draw`` call in numpy.  seeds [S] ints; calls [S] int64 (the state before the call); probs [S, 2]
    float32 (p_self, p_strong); lens [S] int32; scores [S, P] float32; slots [S, P] int32; alive [S n] or None; counts
    [S, 3] / snap_counts [S P] int64: the accumulators before the call (default zeros).  Returns a dict: "policy2"
    uint8, "policy", "snap" int32 [S n], "opp_inc" float64 [S n, 2], "counts", "snap_counts", "calls" (after)."""
    scores, slots = np.asarray(scores, np.float32), np.asarray(slots, np.int32)
    probs = np.asarray(probs, np.float32)
    S, P = scores.shape
    n = int(n)
    policy2 = np.empty(S * n, np.uint8)
    policy = np.full(S * n, -1, np.int32)
    snap = np.full(S * n, -1, np.int32)
    inc = np.empty((S * n, 2), np.float64)
    counts = np.zeros((S, 3), np.int64) if counts is None else np.array(counts, np.int64).reshape(S, 3)
    snap_counts = np.zeros(S * P, np.int64) if snap_counts is None else np.array(snap_counts, np.int64).reshape(S * P)
    calls = np.array(calls, np.int64)
    live = np.ones(S * n, bool) if alive is None else np.asarray(alive).reshape(S * n) != 0
    for m in range(S):
        rows = slice(m * n, (m + 1) * n)
        w = draw_words(seeds[m], KEY_OPP, n, calls[m])
        L = min(max(int(lens[m]), 0), P)
        cum = np.cumsum(scores[m, :L].astype(np.float64))  # in index order
        total = cum[-1] if L else 0.0
        can_sp = L > 0 and np.isfinite(total) and total > 0
        sp = (u24(w[:, 0]) < probs[m, 0]) if can_sp else np.zeros(n, bool)
        strong = ~sp & (u24(w[:, 1]) < probs[m, 1])
        policy2[rows] = np.where(sp, N.POLICY_EXTERNAL, np.where(strong, N.POLICY_BASIC_STRONG, N.POLICY_BASIC_WEAK))
        if can_sp:
            t = u53(w[:, 2], w[:, 3]) * total
            hit = cum[None, :] > t[:, None]
            k = np.where(hit.any(1), hit.argmax(1), L - 1)
            policy[rows] = np.where(sp, slots[m, k], -1)
            snap[rows] = np.where(sp, m * P + k, -1)
            np.add.at(snap_counts, (m * P + k)[sp & live[rows]], 1)
        inc[rows] = phase_inc(draw_words(seeds[m], KEY_PHASE, n, calls[m]))
        lv = live[rows]
        counts[m] += [int((strong & lv).sum()), int((~sp & ~strong & lv).sum()), int((sp & lv).sum())]
        calls[m] += 1
    return {"policy2": policy2, "policy": policy, "snap": snap, "opp_inc": inc, "counts": counts,
            "snap_counts": snap_counts, "calls": calls}


def collect_law(n, cap, reward, done, snap, alive, pos, size, ep_reward, steps, n_snap):
    """One ``hkl_collect`` call in numpy, but for the row copies themselves: returns where every row goes.  reward
    float32 [S n], done [S n], snap int32 [S n] or None, alive [S n] or None (episode_end="max_steps"), pos / size /
    steps int64 [S] and ep_reward float32 [S n]: the state before the call; n_snap = S pmax.  Returns a dict: "dst"
    int64 [S n] (the ring row of arena i, -1: not stored), "push_pos", "push_n", "pos", "size", "steps", "live" ([S]:
    1 where the member had a running arena), "ep_reward", "tally" [n_snap, 2], "alive" and "count" (None without
    alive)."""
    n, cap = int(n), int(cap)
    reward = np.asarray(reward, np.float32)
    dn = np.asarray(done) != 0
    S = reward.shape[0] // n
    lv = np.ones(S * n, bool) if alive is None else np.asarray(alive) != 0
    pos, size, steps = np.array(pos, np.int64), np.array(size, np.int64), np.array(steps, np.int64)
    dst = np.full(S * n, -1, np.int64)
    push_pos, push_n, live = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
    for m in range(S):
        rows = slice(m * n, (m + 1) * n)
        a = lv[rows]
        cnt = int(a.sum())
        if 0 <= pos[m] < cap:
            rank = np.cumsum(a) - 1
            dst[rows] = np.where(a, m * cap + (pos[m] + rank) % cap, -1)
            push_pos[m], push_n[m] = pos[m], cnt
            pos[m] = (pos[m] + cnt) % cap
            size[m] = min(max(size[m], 0) + cnt, cap)
        steps[m] += cnt
        live[m] = cnt > 0
    ep = np.asarray(ep_reward, np.float32) + np.where(lv, reward, np.float32(0))
    tally = np.zeros((n_snap, 2), np.int64)
    if snap is not None:
        sn = np.asarray(snap, np.int64)
        hit = lv & dn & (sn >= 0) & (sn < n_snap)
        np.add.at(tally, (sn[hit], np.where(reward[hit] > 0, 0, 1)), 1)
    out = {"dst": dst, "push_pos": push_pos, "push_n": push_n, "pos": pos, "size": size, "steps": steps, "live": live,
           "ep_reward": ep, "tally": tally, "alive": None, "count": None}
    if alive is not None:
        after = lv & ~dn
        out["alive"] = after.astype(np.uint8)
        out["count"] = after.reshape(S, n).sum(1).astype(np.int32)
    return out


def clear_episode_words(env, n_rows, device, zeros=None):
    """Clear the episode words of an env's ``n_rows`` arenas (``set_state(aux=0)``: the has-puck timers, time, done,
    winner), which a reset carries over from the games before.  An env without ``set_state`` is left as it is.
    Returns the zero words it used, for the caller to keep and pass back as ``zeros`` (the copy is asynchronous)."""
    if hasattr(env, "set_state"):
        if zeros is None:
            zeros = torch.zeros((n_rows, N.AUX_DIM), dtype=torch.int32, device=device)
        env.set_state(aux=zeros)
    return zeros


def phase_rows(seed, n, rnd=0):
    """The three BasicOpponent starting phases of a member's n arenas in its round ``rnd``: U(0, pi) from a generator
    of the member's own."""
    return np.random.default_rng([int(seed) & U64, PHASE_TAG, int(rnd)]).uniform(0.0, math.pi, (int(n), 3))


# ---------------------------------------------------------------------------------------------------- Collector
class Collector:
    """A round's collection for S members of ``rows_per_member`` arenas each on one env of S n arenas.

    env: a VecHockeyEnv-shaped batch (None: ``store`` only).  bank / explorer: player 1's PolicyBank and its
    ``hockey_amd.explore.Explorer`` (None: the caller fills ``act8[:, :4]``).  mix: a ``PopulationOpponentMix`` of the
    same S members with sampling="arena".  ring: a ``PopulationRing`` / ``PopulationPrioritizedRing`` of S members.
    members: the members' seeds (ints, or objects with ``seed`` such as ``explore.Member``).  backend: "hip" (the
    kernels), "torch" (the laws in numpy) or "auto" ("hip" on a GPU with the library built).  episode_end: "max_steps"
    or "done"; poll_every: under "done", the steps between two reads of the survivors' count.

    A round is ``begin_round(obs, obs2, max_steps)``, ``run_round()`` (or ``step()`` by hand) and ``end_round(actors,
    episodes)``.  The state lives on the device: ``obs`` / ``obs2`` (the observations the next step acts on), ``act8``,
    ``policy2`` / ``policy`` / ``snap`` / ``opp_inc`` (the last draw), ``alive`` (uint8), ``ep_reward``, ``count``
    (int32 [S]), ``steps`` / ``live`` (int64 [S], this round's), ``counts`` [S, 3], ``snap_counts`` [S P], ``tally``
    [max_steps, S P, 2] and ``calls`` [S]."""

    def __init__(self, env, bank, mix, ring, explorer, members, rows_per_member, backend="auto",
                 episode_end="max_steps", poll_every=16):
        self.env, self.bank, self.mix, self.ring, self.explorer = env, bank, mix, ring, explorer
        self.seeds = [int(getattr(m, "seed", m)) & U64 for m in members]
        S, n = len(self.seeds), int(rows_per_member)
        if not 1 <= S <= GROUP_MAX:
            raise ValueError(f"a Collector has 1 to {GROUP_MAX} members, got {S}")
        if n < 1 or n > ring.cap:
            raise ValueError(f"rows_per_member must lie in [1, the ring's capacity {ring.cap}], got {n}")
        if mix.S != S or mix.n_per != n or ring.S != S:
            raise ValueError("the mix, the ring and the Collector have the same members and arenas per member")
        if mix.sampling != "arena":
            raise ValueError("the Collector draws a snapshot per arena and step: the mix must have sampling='arena'")
        if episode_end not in ("max_steps", "done"):
            raise ValueError("episode_end must be 'max_steps' or 'done'")
        dev = self.device = torch.device(ring.device)
        self.backend = resolve_backend(backend, dev)
        if int(poll_every) < 1:
            raise ValueError("poll_every must be positive")
        self.S, self.n, self.N, self.P = S, n, S * n, int(mix.pmax)
        self.stop_at_done, self.poll_every = episode_end == "done", int(poll_every)
        self.prioritized = hasattr(ring, "pers")
        NN, P = self.N, self.P

        def z(shape, dt):
            return torch.zeros(shape, dtype=dt, device=dev)

        self.seeds_t = torch.from_numpy(np.array(self.seeds, np.uint64).view(np.int64)).to(dev)
        self.calls = z(S, torch.int64)
        self.probs, self.len_t = z((S, 2), torch.float32), z(S, torch.int32)
        self.scores, self.slots = z((S, P), torch.float32), z((S, P), torch.int32)
        self.policy2, self.policy, self.snap = z(NN, torch.uint8), z(NN, torch.int32), z(NN, torch.int32)
        self.opp_inc = z((NN, 2), torch.float64)
        self.counts, self.snap_counts = z((S, 3), torch.int64), z(S * P, torch.int64)
        self.obs, self.obs2 = z((NN, 18), torch.float32), z((NN, 18), torch.float32)
        self.act8 = z((NN, 8), torch.float32)
        self.alive, self.ep_reward = torch.ones(NN, dtype=torch.uint8, device=dev), z(NN, torch.float32)
        self.push_pos, self.push_n = z(S, torch.int64), z(S, torch.int64)
        self.count = torch.full((S,), n, dtype=torch.int32, device=dev)
        self.steps, self.live = z(S, torch.int64), z(S, torch.int64)
        self.tally, self.t, self.any_pool = None, 0, False
        self._scratch = self._dio = self._cio = self._aux0 = None
        if self.backend == "hip":
            from . import learner_hip as LH

            if dev.type != "cuda":
                raise N.HockeyNativeError("Collector backend='hip' runs on the GPU only")
            self._scratch = z(int(LH.lib().hkl_collect_scratch_ints(NN, n)), torch.int32)
        self.rounds = 0
        self._set_phases()

    # ------------------------------------------------------------------ a round
    def _set_phases(self):
        """The bots' three phase rows of every arena, keyed by the member's seed and its round: at construction, and
        again at every round's start -- the phases walk with every step the env takes, the steps after a member's last
        episode ended included, and how many of those there are depends on the other members and on ``poll_every``."""
        if self.env is not None and hasattr(self.env, "opponent_phase"):
            self.env.opponent_phase(np.concatenate([phase_rows(s, self.n, self.rounds) for s in self.seeds]), rows=3)

    def sync_pools(self):
        """The pools' scores, bank slots and lengths and the curriculum row, into the fixed device buffers the draw
        reads: once per round (both change only at a round's end)."""
        mix = self.mix
        scores, slots, _ = mix._pool_tensors()
        self.scores.copy_(scores)
        self.slots.copy_(slots)
        lens = mix.pool_sizes()
        self.any_pool = any(lens)
        self.len_t.copy_(torch.tensor(lens, dtype=torch.int32))
        self.probs.copy_(torch.tensor([[mix.p_self, mix.p_strong]] * self.S, dtype=torch.float32))

    def begin_round(self, obs, obs2, max_steps):
        """Start a round of at most ``max_steps`` steps from the reset observations."""
        if self.tally is None or self.tally.shape[0] < max_steps:
            self.tally = torch.zeros((int(max_steps), self.S * self.P, 2), dtype=torch.int64, device=self.device)
        self.max_steps, self.t = int(max_steps), 0
        if self.rounds:
            self._set_phases()
        self.rounds += 1
        self.obs.copy_(obs)
        self.obs2.copy_(obs2)
        for t in (self.ep_reward, self.counts, self.snap_counts, self.tally, self.steps, self.live):
            t.zero_()
        self.alive.fill_(1)
        self.count.fill_(self.n)
        self.sync_pools()
        self._calls0 = self.calls.clone()
        self._ecalls0 = None if self.explorer is None else self.explorer.calls.clone()

    def run_round(self):
        """``step()`` until ``max_steps`` or, under episode_end="done", until a poll finds nobody alive."""
        for t in range(self.max_steps):
            self.step()
            if self.stop_at_done and (t + 1) % self.poll_every == 0 and not self.count.cpu().any():
                break

    def end_round(self, actors=None, episodes=0):
        """Close the round: the call counters to their composition-independent values (module docstring), the counts
        and the tally through the mix's round-end fold (``PopulationOpponentMix.end_round(actors, episodes)``).
        Returns (arena-steps per member as a list, ep_reward [N] on the device, the mix's per-member opponent dicts)."""
        if self.stop_at_done:
            self.calls.copy_(self._calls0 + self.live)
            if self.explorer is not None:
                self.explorer.calls.copy_(self._ecalls0 + self.live)
            self._aux0 = clear_episode_words(self.env, self.N, self.device, self._aux0)
        mix = self.mix
        mix._counts, mix._snap_counts = self.counts.clone(), self.snap_counts.clone()
        mix._outcomes = list(self.tally[:self.t].unbind(0)) if self.any_pool else []
        opp = mix.end_round(actors, episodes)
        return self.steps.cpu().tolist(), self.ep_reward, opp

    # ------------------------------------------------------------------ one step
    @torch.no_grad()
    def step(self):
        """One collection step of every arena (module docstring); returns the env's step result."""
        if self.explorer is not None:
            self.explorer.explore(self.obs, self.act8, 0, count=self.count if self.stop_at_done else None)
        self.draw()
        if self.any_pool:  # every self-play arena of every member: one acting call into player 2's columns
            self.mix.bank.act(self.obs2, self.policy, out=self.act8, out_col=4, backend=self.mix.backend)
        res = self.env.step(self.act8, with_agent_two=True, policy2=self.policy2, opp_inc=self.opp_inc)
        self.store(res.obs, res.obs2, res.reward, res.done)
        return res

    def draw(self):
        """``hkl_opp_draw``: this step's ``policy2`` / ``policy`` / ``snap`` / ``opp_inc`` and the counts."""
        alive = self.alive if self.stop_at_done else None
        if self.backend == "hip":
            from . import learner_hip as LH

            if self._dio is None:
                io = self._dio = LH.OppDrawIO()
                io.n_rows, io.rows_per_member, io.pmax = self.N, self.n, self.P
                for k, t in (("seeds", self.seeds_t), ("calls", self.calls), ("probs", self.probs),
                             ("len", self.len_t), ("scores", self.scores), ("slots", self.slots),
                             ("policy2", self.policy2), ("policy", self.policy), ("snap", self.snap),
                             ("opp_inc", self.opp_inc), ("counts", self.counts), ("snap_counts", self.snap_counts)):
                    setattr(io, k, t.data_ptr())
                io.alive = None if alive is None else alive.data_ptr()
            LH.check(LH.lib().hkl_opp_draw(ctypes.byref(self._dio), LH.stream_ptr(self.device)), "hkl_opp_draw")
            return
        c = lambda t: t.cpu().numpy()  # noqa: E731
        r = opp_draw_law(self.seeds, self.n, c(self.calls), c(self.probs), c(self.len_t), c(self.scores),
                         c(self.slots), None if alive is None else c(alive), c(self.counts), c(self.snap_counts))
        for k in ("policy2", "policy", "snap", "opp_inc", "counts", "snap_counts", "calls"):
            getattr(self, k).copy_(torch.from_numpy(r[k]))

    def store(self, obs_next, obs2_next, reward, done):
        """``hkl_collect`` (and the prioritized members' ``hkl_per_push_group``) on the step's outputs: the transition
        (``obs``, ``act8[:, :4]``, reward, obs_next, done) of every running arena into the ring, the bookkeeping, and
        ``obs`` / ``obs2`` := obs_next / obs2_next."""
        if self.t >= self.tally.shape[0]:
            raise RuntimeError("more steps than begin_round's max_steps")
        ring, alive = self.ring, self.alive if self.stop_at_done else None
        if self.backend == "hip":
            from . import learner_hip as LH

            if reward.dtype != torch.float32 or done.dtype != torch.uint8 or not obs_next.is_contiguous():
                raise ValueError("the step's outputs must be float32 rewards, uint8 done flags and contiguous rows")
            if self._cio is None:
                io = self._cio = LH.CollectIO()
                io.n_rows, io.rows_per_member, io.pmax = self.N, self.n, self.P
                io.act_ld, io.cap = self.act8.stride(0), ring.cap
                for k, t in (("obs", self.obs), ("act", self.act8), ("snap", self.snap), ("s", ring.s), ("a", ring.a),
                             ("r", ring.r), ("s2", ring.s2), ("d", ring.d), ("pos", ring.pos_t), ("size", ring.size_t),
                             ("ep_reward", self.ep_reward), ("push_pos", self.push_pos), ("push_n", self.push_n),
                             ("count", self.count), ("steps", self.steps), ("live", self.live),
                             ("keep_obs", self.obs), ("keep_obs2", self.obs2), ("scratch", self._scratch)):
                    setattr(io, k, t.data_ptr())
                io.alive = None if alive is None else alive.data_ptr()
            io = self._cio
            io.obs_next, io.obs2_next = obs_next.data_ptr(), obs2_next.data_ptr()
            io.reward, io.done = reward.data_ptr(), done.data_ptr()
            io.tally = self.tally[self.t].data_ptr()
            LH.check(LH.lib().hkl_collect(ctypes.byref(io), LH.stream_ptr(self.device)), "hkl_collect")
        else:
            self._store_torch(obs_next, obs2_next, reward, done, alive)
        if self.prioritized:  # the new transitions' priorities, from the device arrays the store left
            from . import learner_hip as LH

            LH.check(ring._L.hkl_per_push_group(ring.pers, ring._pers_dev.data_ptr(), self.push_pos.data_ptr(),
                                                self.push_n.data_ptr(), ring.size_t.data_ptr(), self.n, self.S,
                                                LH.stream_ptr(self.device)), "hkl_per_push_group")
        self.t += 1

    def _store_torch(self, obs_next, obs2_next, reward, done, alive):
        ring, dev = self.ring, self.device
        c = lambda t: t.cpu().numpy()  # noqa: E731
        r = collect_law(self.n, ring.cap, c(reward), c(done), c(self.snap), None if alive is None else c(alive),
                        c(ring.pos_t), c(ring.size_t), c(self.ep_reward), c(self.steps), self.S * self.P)
        dst = torch.from_numpy(r["dst"]).to(dev)
        rows = torch.nonzero(dst >= 0).squeeze(1)
        at = dst[rows]
        ring.s[at], ring.a[at] = self.obs[rows], self.act8[rows, :4]
        ring.r[at], ring.s2[at] = reward[rows].float(), obs_next[rows]
        ring.d[at] = (done[rows] != 0).float()
        for k, t in (("push_pos", self.push_pos), ("push_n", self.push_n), ("pos", ring.pos_t), ("size", ring.size_t),
                     ("steps", self.steps), ("ep_reward", self.ep_reward), ("tally", self.tally[self.t])):
            t.copy_(torch.from_numpy(r[k]))
        self.live += torch.from_numpy(r["live"]).to(dev)
        if alive is not None:
            alive.copy_(torch.from_numpy(r["alive"]))
            self.count.copy_(torch.from_numpy(r["count"]))
        self.obs.copy_(obs_next)
        self.obs2.copy_(obs2_next)


__all__ = ["Collector", "collect_law", "opp_draw_law", "phase_rows", "KEY_OPP", "KEY_PHASE"]

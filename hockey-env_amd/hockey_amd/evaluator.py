"""Evaluation on the device: every member's games against every opponent as ONE batch of arenas.

``evaluate()`` plays one policy against one bot: it builds an env, steps it up to 251 times with an eager actor
forward and about ten small torch launches of bookkeeping per step, and reads ``live.any()`` back every step.  A
population's evaluation is that, once per member and bot.  Every piece of the loop is a function of one arena row and
a few words per cell, so here S members x O opponents x n games -- or a whole cross-play table -- are one batch:

* a *cell* is one (player 1 policy, player 2 opponent, seed) combination playing n = episodes x replicas games; C cells
  side by side are N = C n arenas, cell c owning rows [c n, (c + 1) n), local(i) = i - c n;
* player 1 acts through ``PolicyBank.act`` with a policy per row (``hkl_act``), a cell's player 2 is the weak or the
  strong fused bot (the step kernel's per-arena ``policy2``) or another bank slot;
* the accounting -- returns, lengths, winners, the survivors' count, the bots' phase increments -- is three entry
  points of the learner library (include/hockey_eval.h, csrc/hkl_eval.h): ``hkl_eval_begin``, one ``hkl_eval_step``
  after each step of the env, one ``hkl_eval_fold`` at the end.  The host reads the survivors' count every
  ``poll_every`` steps and one small tensor after the fold.

The laws are stated in include/hockey_eval.h and restated here in numpy (``eval_begin_law``, ``eval_step_law``,
``eval_fold_law``): backend="torch" runs them in place of the kernels, on any device -- slow, and the executable
specification the GPU tests hold the kernels to, word for word.

Game g = r * episodes + e of cell c is reset as ``reset(seed=seeds[c] + e)`` with the puck side ``e % 2 == 1``
(``evaluate()``'s placements) and its bots start at the phases ``evaluate(seed, phase_seed)`` draws, so a bot cell
starts exactly where ``evaluate`` starts it.

Composition independence: ``hkl_act``, the step kernel with given ``opp_inc`` and external actions, ``reset_seeded``
and the draws of this module are all independent of a row's position in the batch, so a cell's games are the same bits
alone and in any batch -- with ``explore="device"`` and ``collect="device"`` a member's evaluations, hence its best
checkpoint, do not depend on who else is in the process.

The one batched difference from ``evaluate()``: the bots' phase increments come from the cell's own stream -- Philox
keyed by ``seeds[c] ^ KEY_PHASE`` at counter (local(i), step) -- not from the step kernel's stream keyed by the global
arena id.  This is statistical only.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .collect import clear_episode_words
from .constants import Mode
from .evaluate import reset_params, tournament_pairs
from .philox_ref import U64, draw_words, phase_inc
from .policy_bank import resolve_backend

KEY_PHASE = 0x6576616C70686173  # HKL_EVAL_KEY_PHASE ("evalphas")
CELLS_MAX = 65535  # HKL_EVAL_CELLS_MAX
FOLD_WG = 256  # hkl_eval_fold's workgroup: the lanes of the return sum's fixed order
_BOTS = {"weak": N.POLICY_BASIC_WEAK, "strong": N.POLICY_BASIC_STRONG}


# ---------------------------------------------------------------------------------------------------- the laws in numpy
def eval_inc(seed, n, t):
    """inc(c, local, t) for local = 0 .. n - 1 of a cell with ``seed``: float64 [n, 2]."""
    return phase_inc(draw_words(seed, KEY_PHASE, n, t))


def eval_begin_law(seeds, n):
    """``hkl_eval_begin`` in numpy for the cells with ``seeds`` of ``n`` rows each: the state dict the other two laws
    take -- "live" uint8, "ret" float64, "length" int32, "winner" int8 [C n], "count" int32 [C], "step" int64 [1],
    "opp_inc" float64 [C n, 2]."""
    C, n = len(seeds), int(n)
    return {"live": np.ones(C * n, np.uint8), "ret": np.zeros(C * n, np.float64), "length": np.zeros(C * n, np.int32),
            "winner": np.zeros(C * n, np.int8), "count": np.full(C, n, np.int32), "step": np.zeros(1, np.int64),
            "opp_inc": np.concatenate([eval_inc(s, n, 0) for s in seeds])}


def eval_step_law(seeds, n, state, reward, done, info0):
    """One ``hkl_eval_step`` call in numpy: ``state`` (eval_begin_law's dict) before the call, reward float32 [C n],
    done [C n], info0 float32 [C n] (the winner column).  Returns the state after it."""
    C, n = len(seeds), int(n)
    live = np.asarray(state["live"]) != 0
    dn = np.asarray(done) != 0
    f = np.asarray(info0, np.float32)
    t = int(state["step"][0])
    fin = live & dn
    with np.errstate(invalid="ignore", over="ignore"):
        ret = np.where(live, state["ret"] + np.asarray(reward, np.float32).astype(np.float64), state["ret"])
        win = np.where(f > 0, 1, np.where(f < 0, -1, 0)).astype(np.int8)  # a NaN fails both compares
    return {"live": (live & ~dn).astype(np.uint8), "ret": ret,
            "length": (state["length"] + live).astype(np.int32),
            "winner": np.where(fin, win, state["winner"]).astype(np.int8),
            "count": (state["count"] - fin.reshape(C, n).sum(1)).astype(np.int32),
            "step": np.array([t + 1], np.int64),
            "opp_inc": np.concatenate([eval_inc(s, n, t + 1) for s in seeds])}


def eval_fold_law(n, live, ret, length, winner):
    """``hkl_eval_fold`` in numpy: (outcomes int64 [C, 4], length_sum int64 [C], return_sum float64 [C]) over the
    finished rows (live == 0) of each cell of ``n`` rows, the return sum in the kernel's order: lane l of 256 adds its
    rows l, l + 256, ... in increasing order from +0.0, then the lanes are added as a tree, p[l] += p[l + s] for
    s = 128 .. 1."""
    n = int(n)
    lv = (np.asarray(live) != 0).reshape(-1, n)
    C = lv.shape[0]
    w = np.asarray(winner).reshape(C, n)
    fin = ~lv
    outcomes = np.stack([(fin & (w > 0)).sum(1), (fin & (w == 0)).sum(1), (fin & (w < 0)).sum(1), lv.sum(1)],
                        1).astype(np.int64)
    length_sum = np.where(fin, np.asarray(length, np.int64).reshape(C, n), 0).sum(1)
    # a skipped row adds nothing: + 0.0 leaves an accumulator that started at +0.0 as it is
    v = np.where(fin, np.asarray(ret, np.float64).reshape(C, n), 0.0)
    pad = -n % FOLD_WG
    v = np.concatenate([v, np.zeros((C, pad))], 1).reshape(C, -1, FOLD_WG)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.zeros((C, FOLD_WG))
        for k in range(v.shape[1]):
            p = p + v[:, k]
        s = FOLD_WG // 2
        while s >= 1:
            p[:, :s] = p[:, :s] + p[:, s:2 * s]
            s //= 2
    return outcomes, length_sum, p[:, 0].copy()


# ---------------------------------------------------------------------------------------------------- Evaluator
class Evaluator:
    """``n_cells`` cells of ``episodes`` x ``replicas`` games each on one env (module docstring).

    It owns one ``VecHockeyEnv`` of N = n_cells x episodes x replicas arenas with policies ("external", "external")
    and auto_reset=False and every device buffer, allocated once and reused by every ``run``.  env: a ready
    VecHockeyEnv-shaped batch of N arenas instead (the kernel source's host build in the CPU tests); the placements
    then come from the host (``reset_episodes(..., placement="host")``'s) and the bots' phases are set only if it has
    ``opponent_phase``.  backend: "hip" (the kernels), "torch" (the laws in numpy) or "auto" ("hip" on a GPU with the
    library built).  poll_every: the steps between two reads of the survivors' count; the results do not depend on it."""

    def __init__(self, n_cells, episodes, replicas=1, mode=Mode.NORMAL, device="cuda:0", backend="auto", poll_every=16,
                 env=None):
        self.C, self.episodes, self.replicas = int(n_cells), int(episodes), int(replicas)
        if not 1 <= self.C <= CELLS_MAX:
            raise ValueError(f"an Evaluator has 1 to {CELLS_MAX} cells, got {n_cells}")
        if self.episodes < 1 or self.replicas < 1:
            raise ValueError("episodes and replicas must be positive")
        dev = self.device = torch.device(device)
        self.backend = resolve_backend(backend, dev)
        if int(poll_every) < 1:
            raise ValueError("poll_every must be positive")
        self.n = self.episodes * self.replicas
        self.N = self.C * self.n
        if self.N >= 1 << 31:
            raise ValueError("n_cells x episodes x replicas must be below 2**31")
        if self.backend == "hip" and dev.type != "cuda":
            raise N.HockeyNativeError("Evaluator backend='hip' runs on the GPU only")
        self.mode, self.poll_every = mode, int(poll_every)
        self.own_env = env is None
        if self.own_env:
            from .vec_env import VecHockeyEnv

            env = VecHockeyEnv(self.N, keep_mode=True, mode=mode, device=dev, policies=("external", "external"),
                               auto_reset=False)
        self.env = env
        C, NN = self.C, self.N

        def z(shape, dt):
            return torch.zeros(shape, dtype=dt, device=dev)

        self.seeds_t, self.step = z(C, torch.int64), z(1, torch.int64)
        self.live, self.ret, self.length = z(NN, torch.uint8), z(NN, torch.float64), z(NN, torch.int32)
        self.winner, self.count = z(NN, torch.int8), z(C, torch.int32)
        self.opp_inc = z((NN, 2), torch.float64)
        # the fold's three outputs in one buffer: one copy to the host
        self._fold = z(6 * C, torch.int64)
        self.outcomes, self.length_sum = self._fold[:4 * C].view(C, 4), self._fold[4 * C:5 * C]
        self.return_sum = self._fold[5 * C:].view(torch.float64)
        self.act8 = z((NN, 8), torch.float32)
        self.pol1, self.pol2, self.policy2 = z(NN, torch.int32), z(NN, torch.int32), z(NN, torch.uint8)
        self._aux0 = self._io = None
        self.steps = 0  # the env steps of the last run

    def close(self):
        if self.own_env and self.env is not None:
            self.env.close()
        self.env = None

    # ------------------------------------------------------------------ the three calls
    def _call(self, name, reward=None, done=None, info=None):
        from . import learner_hip as LH

        if self._io is None:
            io = self._io = LH.EvalIO()
            io.n_rows, io.rows_per_cell, io.info_ld = self.N, self.n, 1
            for k in ("step", "live", "ret", "length", "winner", "count", "opp_inc", "outcomes", "length_sum",
                      "return_sum"):
                setattr(io, k, getattr(self, k).data_ptr())
            io.seeds = self.seeds_t.data_ptr()
        io = self._io
        if reward is not None:
            if (reward.dtype != torch.float32 or done.dtype != torch.uint8 or info.dtype != torch.float32
                    or info.dim() != 2 or info.stride(1) != 1 or not reward.is_contiguous()
                    or not done.is_contiguous()):
                raise ValueError("the step's outputs must be float32 rewards, uint8 done flags and float32 info rows")
            io.reward, io.done, io.info, io.info_ld = reward.data_ptr(), done.data_ptr(), info.data_ptr(), info.stride(0)
        LH.check(getattr(LH.lib(), name)(ctypes.byref(io), LH.stream_ptr(self.device)), name)

    _STATE = ("live", "ret", "length", "winner", "count", "step", "opp_inc")

    def _state(self):
        return {k: getattr(self, k).cpu().numpy() for k in self._STATE}

    def _put(self, state):
        for k in self._STATE:
            getattr(self, k).copy_(torch.from_numpy(np.ascontiguousarray(state[k])).view_as(getattr(self, k)))

    def begin(self):
        """``hkl_eval_begin`` on the seeds in ``seeds_t``."""
        if self.backend == "hip":
            self._call("hkl_eval_begin")
        else:
            self._put(eval_begin_law(self._seeds, self.n))

    def account(self, reward, done, info):
        """``hkl_eval_step`` on a step's outputs."""
        if self.backend == "hip":
            self._call("hkl_eval_step", reward, done, info)
        else:
            c = lambda t: t.cpu().numpy()  # noqa: E731
            self._put(eval_step_law(self._seeds, self.n, self._state(), c(reward), c(done), c(info)[:, 0]))

    def fold(self):
        """``hkl_eval_fold``, then the one copy: (outcomes [C, 4], length_sum [C], return_sum [C]) as numpy arrays."""
        if self.backend == "hip":
            self._call("hkl_eval_fold")
        else:
            s = self._state()
            o, ls, rs = eval_fold_law(self.n, s["live"], s["ret"], s["length"], s["winner"])
            self.outcomes.copy_(torch.from_numpy(o))
            self.length_sum.copy_(torch.from_numpy(ls))
            self.return_sum.copy_(torch.from_numpy(rs))
        f = self._fold.cpu().numpy()
        C = self.C
        return f[:4 * C].reshape(C, 4).copy(), f[4 * C:5 * C].copy(), f[5 * C:].view(np.float64).copy()

    # ------------------------------------------------------------------ a run
    def _reset(self, seeds, phase_seeds, p2):
        """The placements and the bots' starting phases of every cell; returns the mode's max_timesteps."""
        env, n, E = self.env, self.n, self.episodes
        e = np.tile(np.arange(E, dtype=np.int64), self.replicas)  # game g = r E + e plays placement e
        self._aux0 = clear_episode_words(env, self.N, self.device, self._aux0)
        if self.own_env:
            rows = np.concatenate([np.array([int(s) + int(k) for k in e], dtype=object) for s in seeds])
            env.reset_seeded(list(rows), one_starting=np.tile((e % 2) == 1, self.C))
            max_t = 250 if env.mode == Mode.NORMAL else 80
        else:
            params = []
            for s in seeds:
                p, max_t, _ = reset_params(E, int(s), self.mode)
                params.append(p[e])
            env.reset_params(np.concatenate(params))
        if hasattr(env, "opponent_phase"):
            ph = np.zeros((self.N, 3))
            for c, ps in enumerate(phase_seeds):
                u = np.random.default_rng(ps).uniform(0, 2 * np.pi, (n, 2))
                rows = slice(c * n, (c + 1) * n)
                ph[rows, 0] = u[:, 0]
                # the row player 2's bot walks under a policy2 override: 1 for the strong bot, 2 for the weak
                ph[rows, 2 if p2[c] == "weak" else 1] = u[:, 1]
            env.opponent_phase(ph, rows=3)
        return max_t

    @torch.no_grad()
    def run(self, bank, p1, p2, seeds, phase_seeds=None, per_episode=False):
        """Play every cell to the end.  bank: the PolicyBank whose slots act; p1 [C]: player 1's slot of each cell; p2
        [C]: "weak", "strong" or player 2's slot; seeds [C] ints (cell c's game e is ``reset(seed=seeds[c] + e)``);
        phase_seeds [C]: the seeds of the bots' starting phases (default ``seeds``).

        Returns a dict of [C] arrays: ``win`` / ``draw`` / ``loss`` rates, ``mean_return`` and ``mean_length`` over the
        cell's finished games and ``unfinished`` (0 after a whole run); ``per_episode`` adds ``winner`` int8,
        ``returns`` float64 and ``lengths`` int32, each [C, replicas, episodes]."""
        C, n, dev = self.C, self.n, self.device
        p1, p2, seeds = list(p1), list(p2), [int(s) for s in seeds]
        phase_seeds = seeds if phase_seeds is None else [int(s) for s in phase_seeds]
        if not len(p1) == len(p2) == len(seeds) == len(phase_seeds) == C:
            raise ValueError(f"p1, p2, seeds and phase_seeds take one entry per cell ({C})")
        slot2 = [-1 if isinstance(q, str) else int(q) for q in p2]
        for q in p2:
            if isinstance(q, str) and q not in _BOTS:
                raise ValueError(f"player 2 is 'weak', 'strong' or a bank slot, got {q!r}")
        for k in [int(k) for k in p1] + [k for k in slot2 if k >= 0]:
            if not 0 <= k < bank.capacity or not bank.occupied[k]:
                raise ValueError(f"bank slot {k} is free or outside the bank")
        ids = [_BOTS[q] if isinstance(q, str) else N.POLICY_EXTERNAL for q in p2]
        self.pol1.copy_(torch.from_numpy(np.repeat(np.array(p1, np.int32), n)))
        self.pol2.copy_(torch.from_numpy(np.repeat(np.array(slot2, np.int32), n)))
        self.policy2.copy_(torch.from_numpy(np.repeat(np.array(ids, np.uint8), n)))
        self._seeds = [s & U64 for s in seeds]
        self.seeds_t.copy_(torch.from_numpy(np.array(self._seeds, np.uint64).view(np.int64)))
        any_slot = any(k >= 0 for k in slot2)
        env = self.env
        max_t = self._reset(seeds, phase_seeds, p2)
        obs, obs2 = env.observe()
        self.begin()
        self.steps = 0
        for t in range(max_t + 1):  # the longest episode is max_t + 1 steps (done when time >= max_t)
            bank.act(obs, self.pol1, out=self.act8, out_col=0)
            if any_slot:  # the bot rows carry policy -1: not written
                bank.act(obs2, self.pol2, out=self.act8, out_col=4)
            res = env.step(self.act8, with_agent_two=any_slot, policy2=self.policy2, opp_inc=self.opp_inc)
            obs, obs2 = res.obs, res.obs2
            self.account(res.reward, res.done, res.info)
            self.steps += 1
            if (t + 1) % self.poll_every == 0 and not self.count.cpu().any():
                break
        outcomes, length_sum, return_sum = self.fold()
        fin = (n - outcomes[:, 3]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = {"episodes": n, "win": outcomes[:, 0] / fin, "draw": outcomes[:, 1] / fin,
                   "loss": outcomes[:, 2] / fin, "mean_return": return_sum / fin, "mean_length": length_sum / fin,
                   "unfinished": outcomes[:, 3].copy()}
        if per_episode:
            shape = (C, self.replicas, self.episodes)
            out["winner"] = self.winner.cpu().numpy().reshape(shape)
            out["returns"] = self.ret.cpu().numpy().reshape(shape)
            out["lengths"] = self.length.cpu().numpy().reshape(shape)
        return out


# ---------------------------------------------------------------------------------------------------- convenience
def _bank_of(actors, device):
    from .policy_bank import ACT_MAX_POLICIES, PolicyBank

    bank = PolicyBank(len(actors), device, wide=len(actors) > ACT_MAX_POLICIES)
    bank.replace_many(range(len(actors)), actors)
    return bank


def evaluate_many(actors, episodes=100, seeds=42, opponents=("strong", "weak"), replicas=1, mode=Mode.NORMAL,
                  device="cuda:0", backend="auto", poll_every=16, phase_seeds=None, per_episode=False):
    """``evaluate()``'s protocol for K ``actors`` (Actor modules or state dicts) against each of ``opponents`` in one
    batch of K x O cells.  seeds: one int for all actors or [K] ints; phase_seeds likewise (default ``seeds``).
    Returns ``Evaluator.run``'s arrays shaped [K][O] (the per-episode ones [K][O][replicas][episodes])."""
    K, O = len(actors), len(opponents)
    dev = torch.device(device)
    per = lambda v: [int(v)] * K if np.ndim(v) == 0 else [int(s) for s in v]  # noqa: E731
    seeds = per(seeds)
    phase_seeds = seeds if phase_seeds is None else per(phase_seeds)
    if len(seeds) != K or len(phase_seeds) != K:
        raise ValueError("seeds and phase_seeds take one entry per actor")
    ev = Evaluator(K * O, episodes, replicas, mode, dev, backend, poll_every)
    try:
        r = ev.run(_bank_of(actors, dev), np.repeat(np.arange(K), O), list(opponents) * K, np.repeat(seeds, O),
                   np.repeat(phase_seeds, O), per_episode)
    finally:
        ev.close()
    return {k: v if np.ndim(v) == 0 else v.reshape((K, O) + v.shape[1:]) for k, v in r.items()}


def cross_play(actors, games=20, seed=42, include_bots=True, mode=Mode.NORMAL, device="cuda:0", backend="auto",
               poll_every=16, per_game=False):
    """``tournament()``'s table on the Evaluator: actor i as player 1 against column j -- actor j for j < K, with
    ``include_bots`` the weak bot (column K) and the strong one (column K + 1) -- one cell of ``games`` games per pair, in
    ``tournament_pairs``' order, game g of every pair from ``reset(seed=seed + g)``.  Returns ``tournament_fold``'s
    [K][cols] matrices ``win`` / ``draw`` / ``loss`` / ``mean_length`` / ``score``; ``per_game`` adds ``winner``
    [K][cols][games] int8."""
    K, games = len(actors), int(games)
    p1, p2, _ = tournament_pairs(K, 1, include_bots)  # one entry per cell
    cols = len(p1) // K
    dev = torch.device(device)
    ev = Evaluator(K * cols, games, 1, mode, dev, backend, poll_every)
    try:
        r = ev.run(_bank_of(actors, dev), p1, [int(j) if j >= 0 else ("weak" if j == -1 else "strong") for j in p2],
                   [int(seed)] * (K * cols), per_episode=per_game)
    finally:
        ev.close()
    out = {k: r[k].reshape(K, cols) for k in ("win", "draw", "loss", "mean_length")}
    out["score"] = out["win"] + 0.5 * out["draw"]
    if per_game:
        out["winner"] = r["winner"].reshape(K, cols, games)
    return out


class PopulationEval:
    """The ``evaluator`` of ``train_population``: every member against the strong and the weak bot, ``episodes`` games
    each from ``reset(seed=member seed + e)``, as one ``Evaluator`` of 2 S cells on the training bank (refreshed after
    each round's updates: no weights are packed again).  members: S, or the members themselves.  The Evaluator is built
    at the first call, on the bank's device, and kept.

    ``__call__(agents, bank, episodes_done)`` returns one record per member: ``wr_strong``, ``wr_weak``, ``r_strong``,
    ``r_weak``, ``draw_strong``, ``draw_weak``, ``len_strong``, ``len_weak`` and ``episode``."""

    def __init__(self, members=None, episodes=100, replicas=1, mode=Mode.NORMAL, backend="auto", poll_every=16,
                 env=None):
        self.S = None if members is None else members if isinstance(members, int) else len(members)
        self.episodes, self.replicas, self.mode = int(episodes), int(replicas), mode
        self.backend, self.poll_every, self.env = backend, int(poll_every), env
        self.evaluator = None

    def __call__(self, agents, bank, episodes_done=0):
        S = len(agents)
        if self.S is not None and S != self.S:
            raise ValueError(f"a PopulationEval of {self.S} members was called with {S} agents")
        if self.evaluator is None:
            self.S = S
            self.evaluator = Evaluator(2 * S, self.episodes, self.replicas, self.mode, bank.device, self.backend,
                                       self.poll_every, self.env)
        r = self.evaluator.run(bank, np.repeat(np.arange(S), 2), ["strong", "weak"] * S,
                               np.repeat([int(ag.seed) for ag in agents], 2))
        recs = []
        for j in range(S):
            rec = {"episode": int(episodes_done)}
            for o, opp in enumerate(("strong", "weak")):
                c = 2 * j + o
                rec[f"wr_{opp}"], rec[f"r_{opp}"] = float(r["win"][c]), float(r["mean_return"][c])
                rec[f"draw_{opp}"], rec[f"len_{opp}"] = float(r["draw"][c]), float(r["mean_length"][c])
            recs.append(rec)
        return recs

    def close(self):
        if self.evaluator is not None:
            self.evaluator.close()
            self.evaluator = None


__all__ = ["Evaluator", "PopulationEval", "evaluate_many", "cross_play", "eval_begin_law", "eval_step_law",
           "eval_fold_law", "eval_inc", "KEY_PHASE"]

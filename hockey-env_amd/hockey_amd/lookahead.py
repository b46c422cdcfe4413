"""Lookahead: the simulator as an exact model.  Fork each of M live arenas K times into a workspace, run K
continuations of H steps in one hk_rollout, and read the rewards back -- the live env is never stepped or modified.

    la = Lookahead(env, branches=K, horizon=H)
    out = la.evaluate(src, actions)          # src [M] arena ids of env, actions [H, M, K, 8]
    best = out.returns.argmax(dim=1)         # random-shooting MPC: the branch to take per source arena

The copies are exact (hk_copy_arenas: contacts and warm-start impulses included), so with external actions -- or
fused bots and given ``opp_inc`` -- a branch is the trajectory the live arena itself would take under those actions.
Fused policies that draw on the device (random actions, bot phase increments without ``opp_inc``) draw from the
WORKSPACE arena's stream, which is keyed by its own index (include/hockey.h).

Over a horizon a planner can afford almost no branch ends in a goal, and ``returns`` is a few steps of the closeness
term.  ``evaluate(..., value=vf)`` with a ``hockey_amd.value.ValueFn`` adds the terminal value: ``values`` = V(s_H) of
player 1's observation at the end of every branch (one ``vf.v`` call on the M * K rows) and ``bootstrapped`` =
``bootstrap(returns, dones, values, gamma)`` = returns + gamma^H V(s_H) for the branches that did not end.
"""
import torch

from . import _native as N
from .vec_env import VecHockeyEnv


class LookaheadResult:
    __slots__ = ("rewards", "dones", "winner", "returns", "values", "bootstrapped")

    def __init__(self, rewards, dones, winner, returns, values=None, bootstrapped=None):
        self.rewards, self.dones, self.winner, self.returns = rewards, dones, winner, returns
        self.values, self.bootstrapped = values, bootstrapped


def bootstrap(returns, dones, values, gamma):
    """returns [M, K] f32, dones [H, M, K] (non-zero: done), values [M, K] f32 = V(s_H) -> [M, K] f32: a branch with
    a done step inside the horizon keeps its return (whatever its value entry holds), every other branch gets
    returns + gamma^H values.  Float64 arithmetic, rounded once to float32; any device."""
    H = dones.shape[0]
    ended = (dones != 0).any(dim=0)
    tail = torch.where(ended, torch.zeros_like(values, dtype=torch.float64), values.to(torch.float64))
    return (returns.to(torch.float64) + float(gamma) ** H * tail).to(torch.float32)


class Lookahead:
    def __init__(self, env, branches, horizon, gamma=None, max_sources=None, policies=("external", "external")):
        """env: the live VecHockeyEnv; branches K, horizon H; gamma: discount of ``returns`` (default: TD3Config's);
        max_sources: the most source arenas one evaluate() takes (default: env.n); policies: the workspace's
        players (default both external: ``actions`` drive all 8 action words)."""
        if gamma is None:
            from .td3 import TD3Config

            gamma = TD3Config().gamma
        self.env, self.K, self.H, self.gamma = env, int(branches), int(horizon), float(gamma)
        self.M_max = int(env.n if max_sources is None else max_sources)
        if self.K < 1 or self.H < 1 or self.M_max < 1:
            raise ValueError("branches, horizon and max_sources must be positive")
        n = self.M_max * self.K
        self.ws = VecHockeyEnv(n, keep_mode=env.keep_mode, mode=env.mode, device=env.device, policies=policies,
                               auto_reset=False, vel_ref_semantics=env.vel_ref_semantics)
        d = env.device
        self._act = torch.zeros((self.H, n, N.ACT_DIM), dtype=torch.float32, device=d)
        self._inc = torch.zeros((self.H, n, 2), dtype=torch.float64, device=d)
        self._rew = torch.zeros((self.H, n), dtype=torch.float32, device=d)
        self._done = torch.zeros((self.H, n), dtype=torch.uint8, device=d)
        self._disc = self.gamma ** torch.arange(self.H, dtype=torch.float64, device=d)

    def close(self):
        self.ws.close()

    def evaluate(self, src, actions, opp_inc=None, assume_valid=False, value=None):
        """src: [M] arena ids of the live env (M <= max_sources); actions: [H, M, K, 8]; opp_inc: [H, M, K, 2]
        BasicOpponent phase increments or None.  Returns a LookaheadResult of device tensors:
          rewards [H, M, K] f32, dones [H, M, K] u8   as the step kernel wrote them (done is sticky: after a branch's
                                                      terminal step its reward repeats)
          winner  [M, K] i32                          -1 / 0 / 1 at the end of the horizon
          returns [M, K] f32                          sum over t of gamma^t r_t up to AND INCLUDING the branch's first
                                                      done step (accumulated in float64): the repeated terminal
                                                      reward of the sticky done is not counted.
        value: a hockey_amd.value.ValueFn (or None).  With it, two more fields (None without):
          values [M, K] f32                           V(s_H) = value.v of player 1's observation of the workspace
                                                      arenas after the rollout
          bootstrapped [M, K] f32                     bootstrap(returns, dones, values, gamma)"""
        H, K, ws = self.H, self.K, self.ws
        src = torch.as_tensor(src, device=self.env.device).to(torch.int64).reshape(-1)
        M = src.numel()
        if M < 1 or M > self.M_max:
            raise ValueError(f"evaluate takes 1..{self.M_max} source arenas, got {M}")
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.env.device)
        if a.shape != (H, M, K, N.ACT_DIM):
            raise ValueError(f"actions must have shape ({H}, {M}, {K}, {N.ACT_DIM}), got {tuple(a.shape)}")
        mk = M * K
        self._act[:, :mk] = a.reshape(H, mk, N.ACT_DIM)
        if opp_inc is not None:
            inc = torch.as_tensor(opp_inc, dtype=torch.float64, device=self.env.device)
            if inc.shape != (H, M, K, 2):
                raise ValueError(f"opp_inc must have shape ({H}, {M}, {K}, 2), got {tuple(inc.shape)}")
            self._inc[:, :mk] = inc.reshape(H, mk, 2)
        # arena m * K + k of the workspace = branch k of source m
        ws.fork(src.repeat_interleave(K), None, source=self.env, assume_valid=assume_valid)
        io = N.StepIO()
        io.actions = self._act.data_ptr()
        io.opp_inc = self._inc.data_ptr() if opp_inc is not None else None
        io.reward, io.done = self._rew.data_ptr(), self._done.data_ptr()
        if H == 1:
            ws.step_raw(io)
        else:
            ws.rollout_raw(H, io)
        rewards = self._rew[:, :mk].reshape(H, M, K).clone()
        dones = self._done[:, :mk].reshape(H, M, K).clone()
        _, aux = ws.get_state()
        winner = aux[:mk, 4].reshape(M, K).clone()
        # step t counts while no EARLIER step was done
        d = dones.to(torch.float64)
        before = torch.cumsum(d, dim=0) - d
        live = (before == 0).to(torch.float64)
        returns = (rewards.to(torch.float64) * live * self._disc[:, None, None]).sum(dim=0).to(torch.float32)
        if value is None:
            return LookaheadResult(rewards, dones, winner, returns)
        values = value.v(ws.observe()[0][:mk]).reshape(M, K)
        return LookaheadResult(rewards, dones, winner, returns, values, bootstrap(returns, dones, values, self.gamma))

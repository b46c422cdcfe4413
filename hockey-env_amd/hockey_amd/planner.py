"""Random-shooting MPC for player 1 with the simulator as the exact model and a TD3 agent's value as the tail.

    planner = ShootingPlanner(env, ValueFn(agent), branches=32, horizon=8, sigma=0.3)
    plan = planner.act()                     # plan.action [M, 4]: player 1's action for each live arena

``act`` takes the agent's own action on the live env's current observation as the base, draws K open-loop action
sequences around it (``shooting_candidates``: branch 0 is the base held for H steps, branch k > 0 the base plus
N(0, sigma) noise per step, clamped to [-1, 1]), runs them through ``Lookahead`` against a fused BasicOpponent
simulated inside the rollout, scores every branch by ``returns + gamma^H V(s_H)`` (``LookaheadResult.bootstrapped``)
and returns the first action of the best branch.  The live env is never stepped.

The bot's phase increments inside a branch come from the workspace arena's device stream (hockey_amd.lookahead), so
a branch is one sample of the bot's walk, not the live arena's own future draw.  Branches are open loop: the actor is
not re-queried inside a branch.
"""
import torch

from . import _native as N
from .lookahead import Lookahead

_OPPONENTS = {"basic_weak": "weak", "basic_strong": "strong"}


def shooting_candidates(base, branches, horizon, sigma, generator=None):
    """base [M, 4] -> candidates [H, M, K, 4] on base's device: branch 0 is ``base`` at every step, branch k > 0 is
    clamp(base + sigma * eps[t, m, k], -1, 1) with eps ~ N(0, 1) drawn from ``generator`` (one [H, M, K, 4] draw)."""
    if base.dim() != 2 or base.shape[1] != 4:
        raise ValueError(f"base must be [M, 4], got {tuple(base.shape)}")
    K, H, M = int(branches), int(horizon), base.shape[0]
    if K < 1 or H < 1:
        raise ValueError("branches and horizon must be positive")
    eps = torch.randn((H, M, K, 4), dtype=base.dtype, device=base.device, generator=generator)
    cand = torch.clamp(base[None, :, None, :] + float(sigma) * eps, -1.0, 1.0)
    cand[:, :, 0, :] = base[None]
    return cand


class PlanResult:
    __slots__ = ("action", "branch", "score", "lookahead")

    def __init__(self, action, branch, score, lookahead):
        self.action, self.branch, self.score, self.lookahead = action, branch, score, lookahead


class ShootingPlanner:
    def __init__(self, env, value, branches=32, horizon=8, sigma=0.3, gamma=None, opponent="basic_strong", seed=0,
                 max_sources=None):
        """env: the live VecHockeyEnv; value: a hockey_amd.value.ValueFn on env's device (its actor gives the base
        action, its critics the tail); branches K, horizon H, sigma: the candidates' noise; gamma: the discount
        (default: TD3Config's); opponent: "basic_weak" or "basic_strong", player 2 inside the rollout; seed: of the
        candidates' generator; max_sources: the most arenas one act() plans for (default: env.n)."""
        if opponent not in _OPPONENTS:
            raise ValueError(f"opponent must be one of {sorted(_OPPONENTS)}, got {opponent!r}")
        self.env, self.value, self.sigma = env, value, float(sigma)
        self.la = Lookahead(env, branches, horizon, gamma=gamma, max_sources=max_sources,
                            policies=("external", _OPPONENTS[opponent]))
        self.K, self.H = self.la.K, self.la.H
        self.generator = torch.Generator(device=env.device)
        self.generator.manual_seed(int(seed))
        self._act8 = torch.zeros((self.H, self.la.M_max, self.K, N.ACT_DIM), dtype=torch.float32, device=env.device)

    def close(self):
        self.la.close()

    def candidates(self, base):
        """[H, M, K, 8] action words of the rollout: player 1's four from shooting_candidates (this planner's
        generator advances), player 2's four zero (the fused bot writes its own)."""
        a8 = self._act8[:, :base.shape[0]]
        a8[..., :4] = shooting_candidates(base, self.K, self.H, self.sigma, self.generator)
        return a8

    @torch.no_grad()
    def act(self, src=None):
        """Plan for the live arenas ``src`` ([M] ids; all when None).  Returns a PlanResult: action [M, 4] (the
        chosen branch's first action), branch [M] = score.argmax(1), score [M, K] = the bootstrapped returns, and the
        LookaheadResult."""
        env = self.env
        if src is None:
            src = torch.arange(env.n, device=env.device)
        src = torch.as_tensor(src, device=env.device).to(torch.int64).reshape(-1)
        if src.numel() < 1 or src.numel() > self.la.M_max:
            raise ValueError(f"act plans for 1..{self.la.M_max} arenas, got {src.numel()}")
        obs =env.observe()[0][src]
        _, base = self.value.v(obs, return_action=True)
        a8 = self.candidates(base)
        out = self.la.evaluate(src, a8, value=self.value)
        score = out.bootstrapped
        branch = score.argmax(dim=1)
        action = a8[0, torch.arange(src.numel(), device=env.device), branch, :4].clone()
        return PlanResult(action, branch, score, out)

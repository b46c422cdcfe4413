"""hockey_amd -- MI355X-native batched air-hockey simulator (drop-in for julilili42/hockey-env's hot path).

Public surface:
  VecHockeyEnv                      N arenas on one GPU, torch tensors in/out (hockey_amd.vec_env)
  HockeyEnv, HockeyEnv_BasicOpponent, BasicOpponent, Mode, make
                                    the reference's single-env API (hockey_amd.hockey_env)
  ArenaSnapshot, Lookahead          exact arena snapshots (VecHockeyEnv.snapshot / restore / fork) and K-way
                                    lookahead over forked arenas (hockey_amd.snapshot, hockey_amd.lookahead)
  ValueFn, ShootingPlanner          a TD3 agent's twin-critic values Q(s, a) / V(s) on batches, and random-shooting
                                    MPC on value-bootstrapped lookahead (hockey_amd.value, hockey_amd.planner)
  PopulationLearner, PopulationRing, train_population
                                    up to 64 TD3 agents trained in one process on the grouped learner kernels
                                    (hockey_amd.population)
The compute path is libhockey_hip.so (csrc/, C ABI in include/hockey.h); torch only provides device
memory and streams.
"""
from .constants import Mode  # noqa: F401


def __getattr__(name):
    if name == "VecHockeyEnv":
        from .vec_env import VecHockeyEnv
        return VecHockeyEnv
    if name in ("HockeyEnv", "HockeyEnv_BasicOpponent", "BasicOpponent", "make", "register_envs"):
        from . import hockey_env
        return getattr(hockey_env, name)
    if name == "ArenaSnapshot":
        from .snapshot import ArenaSnapshot
        return ArenaSnapshot
    if name == "Lookahead":
        from .lookahead import Lookahead
        return Lookahead
    if name == "ValueFn":
        from .value import ValueFn
        return ValueFn
    if name == "ShootingPlanner":
        from .planner import ShootingPlanner
        return ShootingPlanner
    if name in ("PopulationLearner", "PopulationRing", "train_population"):
        from . import population
        return getattr(population, name)
    raise AttributeError(name)

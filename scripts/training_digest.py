#!/usr/bin/env python3
"""One sha256 per training case: a refactor of the training loops must leave every line as it was.

Each case runs ``hockey_amd.td3.train`` or ``hockey_amd.population.train_population`` on a tiny job and hashes every
tensor its ``on_step`` hook sees, the final ``checkpoint()`` tensors of every agent, ``repr(stats)`` without
``round_time`` and every self-play pool's scores and bank slots.  ``collect="device"`` refuses ``on_step`` and a ready
mix: those cases hash the replay ring's tensors and positions instead.  Only the public API is used, so the same file
runs on an older commit; run it on both, on the same machine, and compare the lines.

Every ``episode_end="done"`` case runs at ``max_steps=120`` and asserts that episodes did end before it prints its
line (fewer arena-steps than rounds x arenas x max_steps).  The ``explore="device"``, ``collect="device"`` and
``evaluator=`` cases run, on the CPU, on the numpy laws of hockey_amd.explore / collect / evaluator.

On the CPU (the default) the env is the kernel source's host build (tests/hostcheck.py HostTorchEnv).  With
``--device cuda:0`` the env is a VecHockeyEnv and three cases are added: ``train`` on the fused learner with graph
capture (uniform replay and the device prioritized sampler) and a population of three on the wide policy bank; the
population cases then run at batch 256, because a population on the GPU always uses the fused learner; a fourth is
a ``collect="device"`` population with a prioritized member under graph capture.  Lines of the eager torch learner on
the GPU need not repeat from run to run; every fused-learner line does.

    python scripts/training_digest.py [--device cuda:0] [--only SUBSTRING]
"""
import argparse
import contextlib
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "hockey-env_amd")]

import torch  # noqa: E402

import hockey_amd.opponents as opponents  # noqa: E402
import hockey_amd.population as population  # noqa: E402
from hockey_amd.population import train_population  # noqa: E402
from hockey_amd.td3 import TD3Config, train  # noqa: E402

TABLE = [(1.0, 0.3, 0.3, 0.4)]
N, ROUNDS = 8, 4
BASE = dict(max_steps=30, start_steps=100, batch_size=32, self_play_interval=8, self_play_pool_size=2, buffer_size=400)
DONE = dict(max_steps=120, buffer_size=1000)  # episode_end="done": long enough for episodes to end


class _Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def text(self, s):
        self.h.update(s.encode())

    def tensor(self, t):
        t = t.detach().cpu().contiguous()
        self.text(f"{t.dtype}{tuple(t.shape)}")
        self.h.update(t.numpy().tobytes())

    def on_step(self, *args):
        for a in args:
            if torch.is_tensor(a):
                self.tensor(a)

    def agent(self, agent):
        for net, sd in sorted(agent.checkpoint().items()):
            for name, t in sorted(sd.items()):
                self.text(f"{net}/{name}")
                self.tensor(t)

    def stats(self, stats):
        for st in stats if isinstance(stats, list) else [stats]:
            self.text(repr({k: v for k, v in st.items() if k != "round_time"}))

    def pool(self, pool):
        self.text("pool" + (repr((pool.scores, pool.slots, pool.episode_counter)) if pool is not None else "None"))

    def ring(self, ring):
        for name in ("s", "a", "r", "s2", "d", "pos_t", "size_t", "w"):
            if hasattr(ring, name):
                self.text(name)
                self.tensor(getattr(ring, name))

    def hex(self):
        return self.h.hexdigest()


def _env(n, device):
    if torch.device(device).type != "cpu":
        return None  # train builds its VecHockeyEnv
    from hostcheck import HostTorchEnv

    return HostTorchEnv(n, policies=("external", "external"))


def _eval_env(n, device):
    """The host env an Evaluator steps: a step without agent two carries ``obs2`` None."""
    if torch.device(device).type != "cpu":
        return None  # the Evaluator builds its VecHockeyEnv
    from hostcheck import HostTorchEnv

    class Env(HostTorchEnv):
        def step(self, *a, **k):
            res = super().step(*a, **k)
            if not hasattr(res, "obs2"):
                res.obs2 = None
            return res

    return Env(n, policies=("external", "external"))


@contextlib.contextmanager
def _made(module, *names):
    """train / train_population build their own mix and ring: swap ``module.name`` for a subclass that records its
    instances, and keep a hand on them."""
    made, orig = [], {k: getattr(module, k) for k in names}

    def recording(cls):
        class Rec(cls):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                made.append(self)

        return Rec

    for k, cls in orig.items():
        setattr(module, k, recording(cls))
    try:
        yield made
    finally:
        for k, cls in orig.items():
            setattr(module, k, cls)


def _episodes_ended(stats, rounds, n, max_steps):
    """episode_end="done": a line is only printed by a run in which episodes ended."""
    for st in stats if isinstance(stats, list) else [stats]:
        assert 0 < st["env_steps"] < rounds * n * max_steps, (st["env_steps"], rounds * n * max_steps)


def run_train(device, cfg_kw=None, n=N, rounds=ROUNDS, updates=5, graphs=False, sampling=None,
              episode_end="max_steps", collect="torch", **kw):
    opponents.CURRICULA["digest"] = TABLE
    done = DONE if episode_end == "done" else {}
    cfg = TD3Config(**{**BASE, **done, **(cfg_kw or {})})
    dg = _Digest()
    kw = dict(n_arenas=n, rounds=rounds, device=device, seed=7, updates_per_round=updates, graphs=graphs,
              env=_env(n, device), episode_end=episode_end, collect=collect, **kw)
    if collect == "device":  # no on_step, no ready mix: the ring and train's own mix are hashed
        cfg = TD3Config(**{**BASE, **done, "curriculum_name": "digest", "use_self_play": True, **(cfg_kw or {})})
        with _made(opponents, "PopulationOpponentMix") as mixes, \
                _made(population, "PopulationRing", "PopulationPrioritizedRing") as rings:
            agent, stats = train(cfg=cfg, **kw)
        pools = [p for mix in mixes for p in mix.pools]
    else:
        mix = opponents.OpponentMix(n, TABLE, True, cfg.self_play_interval, cfg.self_play_pool_size, device, 7,
                                    sampling=sampling or "step")
        agent, stats = train(cfg=cfg, on_step=dg.on_step, mix=mix, **kw)
        pools, rings = [mix.pool], []
    if episode_end == "done":
        _episodes_ended(stats, rounds, n, cfg.max_steps)
    dg.agent(agent)
    dg.stats(stats)
    for pool in pools:
        dg.pool(pool)
    for ring in rings:
        dg.ring(ring)
    return dg.hex()


def run_population(device, self_play, episode_end="max_steps", cfg_kw=None, per=(False, False, False), n=N,
                   rounds=ROUNDS, updates=5, graphs=False, collect="torch", evaluate=False, **kw):
    opponents.CURRICULA["digest"] = TABLE
    sp = self_play is not None
    ckw = {**BASE, **(DONE if episode_end == "done" else {}), "curriculum_name": "digest", **(cfg_kw or {})}
    if torch.device(device).type == "cuda":
        ckw["batch_size"] = 256  # a population on the GPU always runs the fused learner: batches of 256
    members = [(TD3Config(noise_mode="gaussian", use_self_play=sp, prioritized_replay=per[0], **ckw), 3),
               (TD3Config(noise_mode="ornstein-uhlenbeck", lr_q=1e-3, use_self_play=sp, prioritized_replay=per[1],
                          **ckw), 11),
               (TD3Config(noise_mode="gaussian", use_self_play=False, prioritized_replay=per[2], **ckw), 5)]
    dg = _Digest()
    if collect != "device":
        kw["on_step"] = dg.on_step
    if evaluate:  # 3 members x 2 bots x 2 games
        from hockey_amd.evaluator import PopulationEval

        kw["evaluator"] = PopulationEval(3, episodes=2, env=_eval_env(12, device))
    with _made(opponents, "PopulationOpponentMix") as mixes, \
            _made(population, "PopulationRing", "PopulationPrioritizedRing") as rings:
        agents, stats = train_population(members, n_arenas=n, rounds=rounds, device=device, env=_env(3 * n, device),
                                         updates_per_round=updates, graphs=graphs, episode_end=episode_end,
                                         self_play=self_play, collect=collect, **kw)
    if evaluate:
        assert [len(st["evals"]) for st in stats] == [1, 1, 1], "one evaluation was due"
        kw["evaluator"].close()
    if episode_end == "done":
        _episodes_ended(stats, rounds, n, ckw["max_steps"])
    for ag in agents:
        dg.agent(ag)
    dg.stats(stats)
    for mix in mixes:
        for pool in mix.pools:
            dg.pool(pool)
    if collect == "device":
        for ring in rings:
            dg.ring(ring)
    return dg.hex()


def cases(device):
    ends = ("max_steps", "done")
    out = [("train default", lambda: run_train(device)),
           ("train self_play_sampling=arena", lambda: run_train(device, sampling="arena")),
           ("train episode_end=done", lambda: run_train(device, episode_end="done")),
           ("train prioritized_replay", lambda: run_train(device, {"prioritized_replay": True})),
           ("train reset=seeded_host", lambda: run_train(device, reset="seeded_host")),
           ("train reset=device", lambda: run_train(device, reset="device"))]
    for sp in (None, "arena", "step"):
        for end in ends:
            out.append((f"population self_play={sp} episode_end={end}",
                        lambda sp=sp, end=end: run_population(device, sp, end)))
    for end in ends:
        out.append((f"train explore=device episode_end={end}",
                    lambda end=end: run_train(device, episode_end=end, explore="device")))
        out.append((f"train explore=device collect=device episode_end={end}",
                    lambda end=end: run_train(device, episode_end=end, explore="device", collect="device")))
        out.append((f"population explore=device self_play=arena episode_end={end}",
                    lambda end=end: run_population(device, "arena", end, explore="device")))
        for sp in (None, "arena"):
            out.append((f"population explore=device collect=device self_play={sp} episode_end={end}",
                        lambda sp=sp, end=end: run_population(device, sp, end, explore="device", collect="device")))
    out.append(("population evaluator", lambda: run_population(device, None, cfg_kw={"eval_interval": 24},
                                                               evaluate=True)))
    if torch.device(device).type == "cuda":
        fused = dict(cfg_kw={"batch_size": 256, "max_steps": 40}, rounds=3, updates=10, graphs=True, fused=True)
        out.append(("fused train graphs uniform", lambda: run_train(device, **fused)))
        fused_per = dict(fused, cfg_kw={**fused["cfg_kw"], "prioritized_replay": True}, per_sampler="device")
        out.append(("fused train graphs per_sampler=device", lambda: run_train(device, **fused_per)))
        # 3 x (21 + 1) = 66 bank slots: past hkl_act's 64, so the mix acts through hkl_act_wide
        wide = {"batch_size": 256, "max_steps": 40, "self_play_pool_size": 21}
        out.append(("fused population graphs per+uniform self_play=arena wide bank",
                    lambda: run_population(device, "arena", cfg_kw=wide, per=(True, False, False), rounds=3,
                                           updates=10, graphs=True)))
        out.append(("fused population graphs per+uniform explore=device collect=device self_play=arena",
                    lambda: run_population(device, "arena", cfg_kw={"batch_size": 256, "max_steps": 40},
                                           per=(True, False, False), rounds=3, updates=10, graphs=True,
                                           explore="device", collect="device")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    args = ap.parse_args()
    torch.set_num_threads(1)  # CPU reductions in one fixed order
    for name, fn in cases(args.device):
        if args.only in name:
            print(f"{fn()}  {name}", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One sha256 per training case: a refactor of the training loops must leave every line as it was.

Each case runs ``hockey_amd.td3.train`` or ``hockey_amd.population.train_population`` on a tiny job and hashes every
tensor its ``on_step`` hook sees, the final ``checkpoint()`` tensors of every agent, ``repr(stats)`` without
``round_time`` and every self-play pool's scores and bank slots.  Only the public API is used, so the same file runs
on an older commit; run it on both, on the same machine, and compare the lines.

On the CPU (the default) the env is the kernel source's host build (tests/hostcheck.py HostTorchEnv).  With
``--device cuda:0`` the env is a VecHockeyEnv and three cases are added: ``train`` on the fused learner with graph
capture (uniform replay and the device prioritized sampler) and a population of three on the wide policy bank; the
population cases then run at batch 256, because a population on the GPU always uses the fused learner.  Lines of the
eager torch learner on the GPU need not repeat from run to run; every fused-learner line does.

    python scripts/training_digest.py [--device cuda:0] [--only SUBSTRING]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "hockey-env_amd")]

import torch  # noqa: E402

import hockey_amd.opponents as opponents  # noqa: E402
from hockey_amd.population import train_population  # noqa: E402
from hockey_amd.td3 import TD3Config, train  # noqa: E402

TABLE = [(1.0, 0.3, 0.3, 0.4)]
N, ROUNDS = 8, 4
BASE = dict(max_steps=30, start_steps=100, batch_size=32, self_play_interval=8, self_play_pool_size=2, buffer_size=400)


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

    def hex(self):
        return self.h.hexdigest()


def _env(n, device):
    if torch.device(device).type != "cpu":
        return None  # train builds its VecHockeyEnv
    from hostcheck import HostTorchEnv

    return HostTorchEnv(n, policies=("external", "external"))


def run_train(device, cfg_kw=None, n=N, rounds=ROUNDS, updates=5, graphs=False, sampling=None, **kw):
    cfg = TD3Config(**{**BASE, **(cfg_kw or {})})
    dg = _Digest()
    mix = opponents.OpponentMix(n, TABLE, True, cfg.self_play_interval, cfg.self_play_pool_size, device, 7,
                                sampling=sampling or "step")
    agent, stats = train(n_arenas=n, rounds=rounds, cfg=cfg, device=device, seed=7, updates_per_round=updates,
                         graphs=graphs, env=_env(n, device), on_step=dg.on_step, mix=mix, **kw)
    dg.agent(agent)
    dg.stats(stats)
    dg.pool(mix.pool)
    return dg.hex()


def run_population(device, self_play, episode_end="max_steps", cfg_kw=None, per=(False, False, False), n=N,
                   rounds=ROUNDS, updates=5, graphs=False):
    opponents.CURRICULA["digest"] = TABLE
    made = []

    class Mix(opponents.PopulationOpponentMix):  # train_population builds its own mix: keep a hand on its pools
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    sp = self_play is not None
    kw = {**BASE, "curriculum_name": "digest", **(cfg_kw or {})}
    if torch.device(device).type == "cuda":
        kw["batch_size"] = 256  # a population on the GPU always runs the fused learner: batches of 256
    members = [(TD3Config(noise_mode="gaussian", use_self_play=sp, prioritized_replay=per[0], **kw), 3),
               (TD3Config(noise_mode="ornstein-uhlenbeck", lr_q=1e-3, use_self_play=sp, prioritized_replay=per[1],
                          **kw), 11),
               (TD3Config(noise_mode="gaussian", use_self_play=False, prioritized_replay=per[2], **kw), 5)]
    dg = _Digest()
    orig, opponents.PopulationOpponentMix = opponents.PopulationOpponentMix, Mix
    try:
        agents, stats = train_population(members, n_arenas=n, rounds=rounds, device=device, env=_env(3 * n, device),
                                         updates_per_round=updates, graphs=graphs, on_step=dg.on_step,
                                         episode_end=episode_end, self_play=self_play)
    finally:
        opponents.PopulationOpponentMix = orig
    for ag in agents:
        dg.agent(ag)
    dg.stats(stats)
    for mix in made:
        for pool in mix.pools:
            dg.pool(pool)
    return dg.hex()


def cases(device):
    out = [("train default", lambda: run_train(device)),
           ("train self_play_sampling=arena", lambda: run_train(device, sampling="arena")),
           ("train episode_end=done", lambda: run_train(device, episode_end="done")),
           ("train prioritized_replay", lambda: run_train(device, {"prioritized_replay": True})),
           ("train reset=seeded_host", lambda: run_train(device, reset="seeded_host")),
           ("train reset=device", lambda: run_train(device, reset="device"))]
    for sp in (None, "arena", "step"):
        for end in ("max_steps", "done"):
            out.append((f"population self_play={sp} episode_end={end}",
                        lambda sp=sp, end=end: run_population(device, sp, end)))
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

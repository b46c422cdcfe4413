#!/usr/bin/env python3
"""Collection on the device (hockey_amd.collect: hkl_opp_draw and hkl_collect around the step kernel) against the
collection step it replaces, which survives unchanged as collect="torch": the opponent draw, the clones, ``store_step``,
the ragged ring push and, under episode_end="done", the per-step host syncs.  Both legs act through ``hkl_explore``
(explore="device").

Measurements, device against torch, in ONE process and one session:
  step        ms per collection step (acting, draw, step kernel, store) at S x 20 arenas for S in --sizes, with and
              without self-play (full pools of 12, P(self-play) 0.3) and with and without prioritized replay; and at
              1 x --rows arenas.  The torch leg is ``train_population``'s loop body, restated line for line on the
              same kinds of objects; the device leg is ``Collector.step``.
  split       the torch leg's step at 8 x 20 with self-play, piece by piece (acting, draw, step kernel, clones, store,
              the "done" syncs), each piece bracketed by a device synchronise: the pieces add up to more than the
              unsynchronised step, they show where it goes.
  round       one ``train_population`` round (8 and 32 members, 20 arenas x 250 steps + 640 updates) and one ``train``
              collection round at --train-arenas arenas: the second round of a two-round run, collection and update
              seconds apart.
The step legs alternate (torch, device, torch, ...) --repeats times, each timing a host clock around --steps steps that
ends in a device synchronise, after a warm-up of both and a reset of the arenas before every timing; the record keeps
every repeat and the medians.  No figure is fixed in advance: a cell in which the device path is slower is recorded as
it is.  Needs the GPU: there is no CPU fallback.

Usage: python scripts/collect_bench.py --out profiles/r21/collect_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))

import torch  # noqa: E402

from hockey_amd.collect import Collector  # noqa: E402
from hockey_amd.explore import Explorer, Member  # noqa: E402
from hockey_amd.opponents import OpponentMix, PopulationOpponentMix  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402
from hockey_amd.population import PopulationPrioritizedRing, PopulationRing, train_population  # noqa: E402
from hockey_amd.td3 import TD3, TD3Config, store_step, train  # noqa: E402
from hockey_amd.vec_env import VecHockeyEnv  # noqa: E402

DEV = "cuda:0"
NOISES = ("gaussian", "ornstein-uhlenbeck", "pink", "uniform")
PAST = 100_000  # total_steps at the start of a timing: past start_steps, inside the schedule
POOL = 12


def _timed(fn, steps, before=None):
    if before is not None:
        before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


class Side:
    """One leg's objects for S x n arenas: env, agents, acting bank and Explorer, mix (pools filled), ring."""

    def __init__(self, S, n, self_play, per, leg):
        dev, N = torch.device(DEV), S * n
        self.S, self.n, self.N, self.leg = S, n, N, leg
        cfgs = [TD3Config(noise_mode=NOISES[j % 4], max_steps=250, use_self_play=self_play,
                          self_play_pool_size=POOL, curriculum_name="stage3", prioritized_replay=per)
                for j in range(S)]
        seeds = [100 + j for j in range(S)]
        agents = [TD3(c, dev, s, max_total_steps=10_000 * 250 * n, n_envs=1) for c, s in zip(cfgs, seeds)]
        self.env = VecHockeyEnv(N, device=dev, policies=("external", "external"), auto_reset=False, seed=seeds[0])
        self.bank = PolicyBank(S, dev)
        self.bank.replace_many(range(S), [ag.actor for ag in agents])
        self.member_of = torch.arange(N, device=dev) // n
        self.ex = Explorer(self.bank, [Member.from_agent(ag) for ag in agents], n,
                           policy=self.member_of.to(torch.int32))
        self.ex.total.fill_(PAST)
        if self_play or leg == "device":
            self.mix = PopulationOpponentMix(cfgs, seeds, n, dev, sampling="arena")
            if self_play:
                for _ in range(POOL):
                    self.mix.snapshot(list(range(S)), [ag.actor for ag in agents])
        else:  # train_population(self_play=None): one OpponentMix over all arenas
            self.mix = OpponentMix(N, "stage3", False, 100, POOL, dev, seeds[0])
        self.mix.update_schedule(0.9)  # stage3's last row: strong 0.35, weak 0.35, self-play 0.30
        cap = 250 * n
        self.ring = (PopulationPrioritizedRing(S, cap, device=dev) if per else PopulationRing(S, cap, device=dev))
        self.act8 = torch.zeros((N, 8), device=dev)
        self.ep_reward = torch.zeros(N, device=dev)
        self.alive = torch.ones(N, dtype=torch.bool, device=dev)
        self.self_play = self_play
        self.col = None
        if leg == "device":
            self.col = Collector(self.env, self.bank, self.mix, self.ring, self.ex, seeds, n, backend="hip")
        self.reset(1)

    def reset(self, steps):
        self.env.reset()
        obs, obs2 = self.env.observe()
        self.obs, self.obs2 = obs.clone(), obs2.clone()
        if self.col is not None:
            self.col.begin_round(self.obs, self.obs2, steps)
        else:
            self.mix.reset_stats()

    def _store(self, rows, res, *row):
        self.ring.push(self.member_of if rows is None else self.member_of[rows], *row)

    def torch_step(self):  # hockey_amd.population.train_population, explore="device", collect="torch"
        a = self.ex.explore(self.obs, self.act8, 0, count=None)[:, :4]
        if self.self_play:
            policy2, _, _ = self.mix.select(self.obs2, out=self.act8)
        else:
            policy2, a2, _ = self.mix.select(self.obs2)
            if a2 is not None:
                self.act8[:, 4:] = a2
        res = self.env.step(self.act8, with_agent_two=True, policy2=policy2)
        o2, r, d = res.obs.clone(), res.reward.clone(), res.done.clone()
        store_step(self._store, self.mix, False, self.alive, self.ep_reward, res, self.obs, a, r, o2, d)
        self.obs, self.obs2 = o2, res.obs2.clone()

    def split(self, steps):
        """The torch step's pieces under episode_end="done", each closed by a synchronise: ms per step and piece."""
        acc = dict.fromkeys(("acting", "draw", "step", "clones", "store", "syncs"), 0.0)

        def lap(key, t0):
            torch.cuda.synchronize()
            acc[key] += time.perf_counter() - t0
            return time.perf_counter()

        self.reset(steps)
        torch.cuda.synchronize()
        for _ in range(steps):
            t = time.perf_counter()
            a = self.ex.explore(self.obs, self.act8, 0, count=None)[:, :4]
            t = lap("acting", t)
            policy2, _, _ = self.mix.select(self.obs2, out=self.act8)
            t = lap("draw", t)
            res = self.env.step(self.act8, with_agent_two=True, policy2=policy2)
            t = lap("step", t)
            o2, r, d = res.obs.clone(), res.reward.clone(), res.done.clone()
            obs2 = res.obs2.clone()
            t = lap("clones", t)
            self.alive.fill_(True)  # every arena stays in the store: the cost of a full step
            store_step(self._store, self.mix, True, self.alive, self.ep_reward, res, self.obs, a, r, o2, d)
            t = lap("store", t)
            self.alive.view(self.S, self.n).sum(1, dtype=torch.int32)
            self.alive.view(self.S, self.n).sum(1).tolist()
            t = lap("syncs", t)
            self.obs, self.obs2 = o2, obs2
        return {k: v * 1e3 / steps for k, v in acc.items()}

    def close(self):
        self.env.close()


def step_cell(S, n, self_play, per, steps, repeats, warmup):
    sides = {leg: Side(S, n, self_play, per, leg) for leg in ("torch", "device")}
    fns = {"torch": sides["torch"].torch_step, "device": sides["device"].col.step}
    for leg, fn in fns.items():
        _timed(fn, warmup, lambda leg=leg: sides[leg].reset(warmup))
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for leg, fn in fns.items():
            times[leg].append(_timed(fn, steps, lambda leg=leg: sides[leg].reset(steps)))
    rec = {"members": S, "arenas_per_member": n, "rows": S * n, "self_play": self_play, "prioritized": per,
           "steps_per_timing": steps}
    rec.update({k + "_ms_per_step": t for k, t in times.items()})
    rec.update({k + "_median": statistics.median(t) for k, t in times.items()})
    rec["torch_over_device"] = rec["torch_median"] / rec["device_median"]
    for s in sides.values():
        s.close()
    torch.cuda.empty_cache()
    return rec


def split_cell(S, n, steps):
    side = Side(S, n, True, False, "torch")
    side.split(30)
    rec = {"members": S, "arenas_per_member": n, "self_play": True, "episode_end": "done", "steps": steps,
           "ms_per_step": side.split(steps), "unsynchronised_step_ms": _timed(side.torch_step, steps,
                                                                              lambda: side.reset(steps))}
    side.close()
    return rec


def population_round(S, arenas=20):
    cfgs = [TD3Config(max_steps=250, use_self_play=False, curriculum_name="noise_study", noise_mode=NOISES[j % 4])
            for j in range(S)]
    rec = {"members": S, "arenas_per_member": arenas, "steps": 250}
    for leg in ("torch", "device"):
        _, st = train_population([(c, 100 + j) for j, c in enumerate(cfgs)], n_arenas=arenas, rounds=2, device=DEV,
                                 timing=True, explore="device", collect=leg)
        c, u = st[0]["round_time"][1]
        rec[leg + "_round_s"] = {"collect": c, "update": u, "total": c + u}
        rec["updates_per_round"] = st[0]["updates_per_round"]
    rec["torch_over_device_collect"] = rec["torch_round_s"]["collect"] / rec["device_round_s"]["collect"]
    rec["torch_over_device_total"] = rec["torch_round_s"]["total"] / rec["device_round_s"]["total"]
    return rec


def train_round(arenas):
    cfg = TD3Config(use_self_play=False, curriculum_name="stage1")
    rec = {"arenas": arenas, "steps": cfg.max_steps, "what": "train(): the second round's collection"}
    for leg in ("torch", "device"):
        _, st = train(n_arenas=arenas, rounds=2, cfg=cfg, device=DEV, seed=5, timing=True, updates_per_round=2,
                      explore="device", collect=leg)
        c, u = st["round_time"][1]
        rec[leg + "_collect_s"] = c
        rec[leg + "_env_steps_per_s"] = arenas * cfg.max_steps / c
        torch.cuda.empty_cache()
    rec["torch_over_device_collect"] = rec["torch_collect_s"] / rec["device_collect_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,32,64")
    ap.add_argument("--round-sizes", default="8,32")
    ap.add_argument("--rows", type=int, default=65536, help="0 skips the one-member wide cell")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--train-arenas", type=int, default=65536, help="0 skips the train() collection round")
    ap.add_argument("--session", default="", help="a label of the measuring session, kept in the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "collect_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collect_bench needs the GPU (no CPU fallback)")
    out = {"what": "collection step: collect='device' (hkl_opp_draw + hkl_collect) against collect='torch' (the "
                   "parent's collection step), both with explore='device'; one process, legs alternated, medians "
                   "over the repeats; every figure measured in this session",
           "session": args.session, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "warmup_steps": args.warmup, "step": [], "split": [], "round": [], "train_round": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def record(key, rec):  # the file is rewritten after every measurement
        out[key].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for S in (int(x) for x in args.sizes.split(",") if x):
        for self_play in (False, True):
            for per in (False, True):
                record("step", step_cell(S, 20, self_play, per, args.steps, args.repeats, args.warmup))
    if args.rows:
        record("step", step_cell(1, args.rows, False, False, args.steps, args.repeats, args.warmup))
    record("split", split_cell(8, 20, args.steps))
    for S in (int(x) for x in args.round_sizes.split(",") if x):
        record("round", population_round(S))
    if args.train_arenas:
        record("train_round", train_round(args.train_arenas))


if __name__ == "__main__":
    main()

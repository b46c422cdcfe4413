#!/usr/bin/env python3
"""Collection on the device (hockey_amd.collect: hkl_opp_draw and hkl_collect around the step kernel) against the
collection step it replaces, which survives unchanged as collect="torch": the opponent draw, the clones, ``store_step``,
the ragged ring push and, under episode_end="done", the per-step host syncs.  Both legs act through ``hkl_explore``
(explore="device").

Measurements, device against torch, in ONE process and one session:
  step        ms per collection step (acting, draw, step kernel, store) at S x 20 arenas for S in --sizes, with and
              without self-play (full pools of 12, P(self-play) 0.3) and with and without prioritized replay; and at
              1 x --rows arenas.  The torch leg is ``hockey_amd.host_round.TorchCollector.step``, the collector of
              ``train_population(collect="torch")``, on the same kinds of objects; the device leg is ``Collector.step``.
  split       the torch leg's step at 8 x 20 with self-play, piece by piece (acting, draw, step kernel, clones, store,
              the "done" syncs), each piece bracketed by a device synchronise: the pieces add up to more than the
              unsynchronised step, they show where it goes.  The pieces are the TorchCollector's own, so from the
              second step on "acting" gets the survivors' count as the library passes it (an int32 device tensor);
              the splits recorded up to profiles/r21 called ``explore`` with ``count=None``.
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
sys.path[:0] = [os.path.join(ROOT, "hockey-env_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import explore_bench  # noqa: E402
from explore_bench import DEV, NOISES, PAST  # noqa: E402

from hockey_amd.collect import Collector  # noqa: E402
from hockey_amd.explore import Explorer, Member  # noqa: E402
from hockey_amd.host_round import TorchCollector  # noqa: E402
from hockey_amd.opponents import OpponentMix, PopulationOpponentMix  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402
from hockey_amd.population import PopulationPrioritizedRing, PopulationRing  # noqa: E402
from hockey_amd.td3 import TD3, TD3Config  # noqa: E402
from hockey_amd.vec_env import VecHockeyEnv  # noqa: E402

POOL = 12
# the round legs are explore_bench's, both acting through hkl_explore
LEGS = {leg: {"explore": "device", "collect": leg} for leg in ("torch", "device")}


def _timed(fn, steps, before):
    before()
    return explore_bench._timed(fn, steps)


class Side:
    """One leg's objects for S x n arenas: env, agents, acting bank and Explorer, mix (pools filled), ring."""

    def __init__(self, S, n, self_play, per, leg):
        dev, N = torch.device(DEV), S * n
        self.leg = leg
        cfgs = [TD3Config(noise_mode=NOISES[j % 4], max_steps=250, use_self_play=self_play,
                          self_play_pool_size=POOL, curriculum_name="stage3", prioritized_replay=per)
                for j in range(S)]
        seeds = [100 + j for j in range(S)]
        agents = [TD3(c, dev, s, max_total_steps=10_000 * 250 * n, n_envs=1) for c, s in zip(cfgs, seeds)]
        self.env = VecHockeyEnv(N, device=dev, policies=("external", "external"), auto_reset=False, seed=seeds[0])
        self.bank = PolicyBank(S, dev)
        self.bank.replace_many(range(S), [ag.actor for ag in agents])
        self.ex = Explorer(self.bank, [Member.from_agent(ag) for ag in agents], n,
                           policy=(torch.arange(N, device=dev) // n).to(torch.int32))
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
        args = (self.env, self.bank, self.mix, self.ring, self.ex, seeds, n)
        self.col = Collector(*args, backend="hip") if leg == "device" else TorchCollector(*args)
        self.torch_step = self.col.step  # the torch leg: train_population(explore="device", collect="torch")'s step
        self.reset(1)

    def reset(self, steps):
        self.env.reset()
        obs, obs2 = self.env.observe()
        if self.leg == "torch":
            self.mix.reset_stats()
        self.col.begin_round(obs.clone(), obs2.clone(), steps)

    def split(self, steps):
        """The torch step's pieces under episode_end="done", each closed by a synchronise: ms per step and piece."""
        acc = dict.fromkeys(("acting", "draw", "step", "clones", "store", "syncs"), 0.0)
        col = self.col

        def lap(key, t0):
            torch.cuda.synchronize()
            acc[key] += time.perf_counter() - t0
            return time.perf_counter()

        col.stop_at_done = True
        self.reset(steps)
        torch.cuda.synchronize()
        for _ in range(steps):  # TorchCollector.step, piece by piece
            t = time.perf_counter()
            a = col.explorer.explore(col.obs, col.act8, 0, count=col.count)[:, :4]
            t = lap("acting", t)
            policy2 = col.draw()
            t = lap("draw", t)
            res = col.env.step(col.act8, with_agent_two=True, policy2=policy2)
            t = lap("step", t)
            row = col.clones(res)
            t = lap("clones", t)
            col.alive.fill_(True)  # every arena stays in the store: the cost of a full step
            col.store_rows(a, res, *row[:3])
            t = lap("store", t)
            col.survivors()
            t = lap("syncs", t)
            col.obs, col.obs2 = row[0], row[3]
        col.stop_at_done = False
        return {k: v * 1e3 / steps for k, v in acc.items()}

    def close(self):
        self.env.close()


def step_cell(S, n, self_play, per, steps, repeats, warmup):
    sides = {leg: Side(S, n, self_play, per, leg) for leg in ("torch", "device")}
    fns = {leg: side.col.step for leg, side in sides.items()}
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
        record("round", explore_bench.population_round(S, legs=LEGS))
    if args.train_arenas:
        record("train_round", explore_bench.train_round(args.train_arenas, LEGS))


if __name__ == "__main__":
    main()

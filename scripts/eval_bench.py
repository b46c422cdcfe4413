#!/usr/bin/env python3
"""Evaluation on the device (hockey_amd.evaluator: all members' games as one batch of arenas on hkl_eval_begin /
hkl_eval_step / hkl_eval_fold) against the serial path it stands beside, which is unchanged: one ``evaluate()`` call per
member and bot, as ``scripts/noise_study.py`` runs it.

Measurements, batched against serial, in ONE process and one session:
  evaluation  one evaluation of S members x {strong, weak} x --episodes episodes for S in --sizes: the serial loop
              (two ``evaluate()`` calls per member, each with its own env) against one ``Evaluator.run`` on a kept
              Evaluator and bank.
  cross_play  ``cross_play`` of --actors actors x --games games against ``tournament`` (both build their env and bank
              inside the call).
  training    --rounds ``train_population`` rounds (explore / collect on "device", 20 arenas x 250 steps) with one
              evaluation at the end, for the member counts in --round-sizes: the ``eval_fn`` path (the serial loop)
              against the ``evaluator`` path (``PopulationEval``); the whole call is timed.
The two paths alternate (serial, batched, serial, ...) --repeats times after a warm-up of both, each timing a host clock
between two device synchronisations; the record keeps every repeat, the median and the spread (min, max).  No figure is
fixed in advance: a cell in which the batched path is slower is recorded as it is.  Needs the GPU: no CPU fallback.

Usage: python scripts/eval_bench.py --out profiles/r22/eval_bench.json
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hockey_amd.evaluate import Actor, evaluate, tournament  # noqa: E402
from hockey_amd.evaluator import Evaluator, PopulationEval, cross_play  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402
from hockey_amd.population import train_population  # noqa: E402
from hockey_amd.td3 import TD3Config  # noqa: E402

DEV = "cuda:0"
NOISES = ("gaussian", "ornstein-uhlenbeck", "pink", "uniform")


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(legs, repeats):
    """Warm every leg once, then time them in turn ``repeats`` times: {leg: seconds per repeat}."""
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(_timed(fn))
    return times


def _summary(rec, times):
    for k, t in times.items():
        rec[k + "_s"] = t
        rec[k + "_median_s"] = statistics.median(t)
        rec[k + "_min_s"], rec[k + "_max_s"] = min(t), max(t)
    rec["serial_over_batched"] = rec["serial_median_s"] / rec["batched_median_s"]
    return rec


def _actors(k, seed=0):
    torch.manual_seed(seed)
    return [Actor().to(DEV).eval() for _ in range(k)]


def serial_eval(actors, seeds, episodes):
    """noise_study's evaluation of a population: per member, evaluate() against the strong, then the weak bot."""
    out = []
    for actor, seed in zip(actors, seeds):
        s = evaluate(actor, episodes=episodes, seed=seed, weak_opponent=False, device=DEV)
        w = evaluate(actor, episodes=episodes, seed=seed, weak_opponent=True, device=DEV)
        out.append((s["win"], w["win"], s["mean_return"], w["mean_return"]))
    return out


def evaluation_cell(S, episodes, repeats):
    actors, seeds = _actors(S, seed=S), [100 + j for j in range(S)]
    bank = PolicyBank(S, DEV)
    bank.replace_many(range(S), actors)
    ev = Evaluator(2 * S, episodes, device=DEV)
    p1, p2, sd = np.repeat(np.arange(S), 2), ["strong", "weak"] * S, np.repeat(seeds, 2)
    last = {}

    def batched():
        last["r"] = ev.run(bank, p1, p2, sd)

    times = _alternate({"serial": lambda: serial_eval(actors, seeds, episodes), "batched": batched}, repeats)
    rec = {"members": S, "episodes": episodes, "cells": 2 * S, "arenas": 2 * S * episodes, "steps": ev.steps,
           "mean_length": float(last["r"]["mean_length"].mean())}
    ev.close()
    torch.cuda.empty_cache()
    return _summary(rec, times)


def cross_play_cell(K, games, repeats):
    actors = _actors(K, seed=7)
    times = _alternate({"serial": lambda: tournament(actors, games=games, seed=42, device=DEV),
                        "batched": lambda: cross_play(actors, games=games, seed=42, device=DEV)}, repeats)
    return _summary({"actors": K, "games": games, "arenas": K * (K + 2) * games,
                     "serial": "tournament()", "batched": "cross_play()"}, times)


def training_cell(S, rounds, episodes, repeats, arenas=20):
    cfgs = [TD3Config(max_steps=250, use_self_play=False, curriculum_name="noise_study", noise_mode=NOISES[j % 4],
                      eval_interval=rounds * arenas) for j in range(S)]
    members = [(c, 100 + j) for j, c in enumerate(cfgs)]

    def eval_fn(agent, ep):
        agent.actor.eval()
        r = serial_eval([agent.actor], [agent.seed], episodes)[0]
        agent.actor.train()
        return r

    def run(rnds, **hook):
        cs = [(dataclasses.replace(c, eval_interval=rnds * arenas), s) for c, s in members]
        _, st = train_population(cs, n_arenas=arenas, rounds=rnds, device=DEV, explore="device", collect="device",
                                 **hook)
        assert all(len(s["evals"]) == 1 for s in st)

    def batched(rnds=rounds):
        pe = PopulationEval(S, episodes=episodes)
        run(rnds, evaluator=pe)
        pe.close()

    for fn in (lambda: run(1, eval_fn=eval_fn), lambda: batched(1)):  # warm-up: one round and one evaluation each
        fn()
    times = {"serial": [], "batched": []}
    for _ in range(repeats):
        times["serial"].append(_timed(lambda: run(rounds, eval_fn=eval_fn)))
        times["batched"].append(_timed(batched))
    torch.cuda.empty_cache()
    return _summary({"members": S, "arenas_per_member": arenas, "rounds": rounds, "evaluations": 1,
                     "episodes": episodes, "what": "the whole train_population call"}, times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,32,64")
    ap.add_argument("--round-sizes", default="8,32")
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--actors", type=int, default=16)
    ap.add_argument("--games", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--session", default="", help="a label of the measuring session, kept in the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs the GPU (no CPU fallback)")
    if args.repeats < 5:
        raise SystemExit("at least five repetitions")
    out = {"what": "evaluation: hockey_amd.evaluator (one batch of arenas on hkl_eval_*) against the serial evaluate() / "
                   "tournament() path; one process, paths alternated after a warm-up of both, host clock between two "
                   "device synchronisations, every repeat kept with the median and the spread; every figure measured "
                   "in this session",
           "session": args.session, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "evaluation": [], "cross_play": [], "training": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def record(key, rec):  # the file is rewritten after every measurement
        out[key].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for S in (int(x) for x in args.sizes.split(",") if x):
        record("evaluation", evaluation_cell(S, args.episodes, args.repeats))
    record("cross_play", cross_play_cell(args.actors, args.games, args.repeats))
    for S in (int(x) for x in args.round_sizes.split(",") if x):
        record("training", training_cell(S, args.rounds, args.episodes, args.repeats))


if __name__ == "__main__":
    main()

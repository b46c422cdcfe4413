#!/usr/bin/env python3
"""Exploration acting on the device (hockey_amd.explore, one hkl_explore call per step) against the acting path it
replaces, which survives unchanged as explore="torch": ``TD3.act`` in ``train`` and its per-member restatement in
``train_population`` (hockey_amd.host_round's two host explorers: host arithmetic, three uploads, ``hkl_act``, the
noise generators, multiply / add / clamp, the random-phase mask, the copy into the step kernel's action columns).

Three measurements, device against torch, in ONE process and one session:
  step        ms per acting step at S x 20 arenas for S in --sizes (the four noise modes in turn over the members,
              past the random phase), the population's path;
  step_wide   ms per acting step at 65 536 rows of one policy, ``train``'s path (gaussian);
  round       one ``train_population`` round (8 and 32 members, 20 arenas x 250 steps + 640 updates) and one ``train``
              collection round at 65 536 arenas: the second round of a two-round run (the first warms up and captures
              the graphs), collection and update seconds apart.
The step legs alternate (torch, device, torch, ...) --repeats times, each timing a host clock around --steps calls
that ends in a device synchronise, after a warm-up of both; the record keeps every repeat and the medians.  The round
legs run once per value (a run is seconds long).  No figure is fixed in advance: a cell in which the device path is
slower is recorded as it is.  Needs the GPU: there is no CPU fallback.

Usage: python scripts/explore_bench.py --out profiles/r20/explore_bench.json
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

from hockey_amd.explore import Explorer, Member  # noqa: E402
from hockey_amd.host_round import AgentExplorer, PopulationExplorer  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402
from hockey_amd.population import train_population  # noqa: E402
from hockey_amd.td3 import TD3, TD3Config, train  # noqa: E402

DEV = "cuda:0"
NOISES = ("gaussian", "ornstein-uhlenbeck", "pink", "uniform")
PAST = 100_000  # total_steps at the start of a timing: past start_steps, inside the schedule


def _timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _alternate(legs, steps, repeats, warmup):
    for fn in legs.values():
        _timed(fn, warmup)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(_timed(fn, steps))
    rec = {k + "_ms_per_step": t for k, t in times.items()}
    rec.update({k + "_median": statistics.median(t) for k, t in times.items()})
    rec["torch_over_device"] = rec["torch_median"] / rec["device_median"]
    return rec


def population_step(S, n, steps, repeats, warmup):
    """One acting step of train_population at S x n arenas: its explore="torch" explorer
    (hockey_amd.host_round.PopulationExplorer) against Explorer.explore, on the same bank."""
    dev, N = torch.device(DEV), S * n
    cfgs = [TD3Config(noise_mode=NOISES[j % 4], max_steps=250) for j in range(S)]
    agents = [TD3(c, dev, 100 + j, max_total_steps=10_000 * 250 * n, n_envs=1) for j, c in enumerate(cfgs)]
    for ag in agents:
        ag.total_steps = PAST
    bank = PolicyBank(S, dev)
    bank.replace_many(range(S), [ag.actor for ag in agents])
    policy = (torch.arange(N, device=dev) // n).to(torch.int32)
    act8 = torch.zeros((N, 8), device=dev)
    obs = torch.randn(N, 18, device=dev)
    host = PopulationExplorer(agents, bank, n)
    ex = Explorer(bank, [Member.from_agent(ag) for ag in agents], n, policy=policy)
    ex.total.fill_(PAST)
    rec = {"members": S, "arenas_per_member": n, "rows": N, "steps_per_timing": steps}
    rec.update(_alternate({"torch": lambda: host.explore(obs, act8, 0), "device": lambda: ex.explore(obs, act8, 0)},
                          steps, repeats, warmup))
    return rec


def wide_step(rows, steps, repeats, warmup):
    """One acting step of train at ``rows`` arenas, one policy: its explore="torch" explorer
    (hockey_amd.host_round.AgentExplorer: TD3.act and the copy) against Explorer.explore."""
    dev = torch.device(DEV)
    agent = TD3(TD3Config(), dev, 3, max_total_steps=10 ** 12, n_envs=rows)
    agent.total_steps = PAST
    bank = PolicyBank(1, dev)
    bank.replace(0, agent.actor)
    ex = Explorer(bank, [Member.from_agent(agent)], rows)
    ex.total.fill_(PAST)
    act8 = torch.zeros((rows, 8), device=dev)
    obs = torch.randn(rows, 18, device=dev)
    host = AgentExplorer(agent)
    rec = {"rows": rows, "policies": 1, "steps_per_timing": steps}
    rec.update(_alternate({"torch": lambda: host.explore(obs, act8, 0), "device": lambda: ex.explore(obs, act8, 0)},
                          steps, repeats, warmup))
    return rec


LEGS = {"torch": {"explore": "torch"}, "device": {"explore": "device"}}  # a round leg's training arguments


def population_round(S, arenas=20, legs=LEGS):
    cfgs = [TD3Config(max_steps=250, use_self_play=False, curriculum_name="noise_study", noise_mode=NOISES[j % 4])
            for j in range(S)]
    rec = {"members": S, "arenas_per_member": arenas, "steps": 250}
    for leg, kw in legs.items():
        _, st = train_population([(c, 100 + j) for j, c in enumerate(cfgs)], n_arenas=arenas, rounds=2, device=DEV,
                                 timing=True, **kw)
        c, u = st[0]["round_time"][1]
        rec[leg + "_round_s"] = {"collect": c, "update": u, "total": c + u}
        rec["updates_per_round"] = st[0]["updates_per_round"]
    rec["torch_over_device_collect"] = rec["torch_round_s"]["collect"] / rec["device_round_s"]["collect"]
    rec["torch_over_device_total"] = rec["torch_round_s"]["total"] / rec["device_round_s"]["total"]
    return rec


def train_round(arenas, legs=LEGS):
    cfg = TD3Config(use_self_play=False, curriculum_name="stage1")
    rec = {"arenas": arenas, "steps": cfg.max_steps, "what": "train(): the second round's collection"}
    for leg, kw in legs.items():
        _, st = train(n_arenas=arenas, rounds=2, cfg=cfg, device=DEV, seed=5, timing=True, updates_per_round=2, **kw)
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
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--train-arenas", type=int, default=65536, help="0 skips the train() collection round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "explore_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explore_bench needs the GPU (no CPU fallback)")
    out = {"what": "exploration acting: explore='device' (one hkl_explore call per step) against explore='torch' "
                   "(the parent's acting path); one process, legs alternated, medians over the repeats; measured",
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup_steps": args.warmup,
           "step": [], "step_wide": [], "round": [], "train_round": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def record(key, rec):  # the file is rewritten after every measurement
        out[key].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for S in (int(x) for x in args.sizes.split(",") if x):
        record("step", population_step(S, 20, args.steps, args.repeats, args.warmup))
    record("step_wide", wide_step(args.rows, args.steps, args.repeats, args.warmup))
    for S in (int(x) for x in args.round_sizes.split(",") if x):
        record("round", population_round(S))
    if args.train_arenas:
        record("train_round", train_round(args.train_arenas))


if __name__ == "__main__":
    main()

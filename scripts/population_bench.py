"""Population learner against the sequence it replaces (hockey_amd.population; DESIGN §3 "Grouped learner kernels").

At the reference's learner batch of 256, for S in --sizes:
  grouped     ms per graph-replayed update pair (critic; critic + actor) of one PopulationLearner of S members;
  sequential  ms for S plain fused Learners replaying their own captured pair one after another in the same process --
              what a seed study could do before the grouped kernels existed.
The two are timed alternately, --repeats times each (--pairs replays per timing, fewer at the large sizes), a device
synchronise around each; the
record holds every repeat and the medians.  --round-sizes adds one full round of training per size: train_population
(20 arenas per member, 250 steps, 640 updates) against S sequential hockey_amd.td3.train rounds, the second round of
each run (the first captures the graphs), collection and update seconds apart.

--prioritized runs the prioritized-replay leg instead (DESIGN §3 "Grouped prioritized replay"), at the same batch and
sizes:
  grouped     one PopulationLearner on a PopulationPrioritizedRing (hkl_per_*_group: 10 + 14 launches per pair);
  sequential  S fused Learners on their own DevicePrioritizedRing replaying their own graphs in turn (the single
              hkl_per_* calls: S x (10 + 14) launches per pair) -- all a population with prioritized replay could do
              before the grouped kernels;
  push        ms per ragged push of one training step's rows (20 arenas per member) into a PopulationPrioritizedRing
              (with priorities: + one hkl_per_push_group) and into a PopulationRing (without), alternated.

No ratio is fixed in advance; the file records what was measured.  Needs the GPU: there is no CPU fallback.

Usage: python scripts/population_bench.py --out profiles/r15/population_bench.json
       python scripts/population_bench.py --prioritized --out profiles/r16/population_per_bench.json
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

from hockey_amd.population import (PopulationLearner, PopulationPrioritizedRing, PopulationRing,  # noqa: E402
                                   train_population)
from hockey_amd.td3 import TD3, DevicePrioritizedRing, Learner, ReplayRing, TD3Config, train  # noqa: E402

DEV = "cuda:0"
B = 256


def _fill(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [t.to(DEV) for t in (torch.randn(n, 18, generator=g), torch.rand(n, 4, generator=g) * 2 - 1,
                                torch.randn(n, generator=g), torch.randn(n, 18, generator=g),
                                (torch.rand(n, generator=g) < 0.05).float())]


def _timed(fn, pairs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(pairs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / pairs


def learner_bench(S, pairs, repeats, cap=8192, prioritized=False):
    pop = PopulationPrioritizedRing(S, cap, device=DEV) if prioritized else PopulationRing(S, cap, device=DEV)
    seq = []
    for j in range(S):
        data = _fill(cap, j)
        pop.push(torch.full((cap,), j, dtype=torch.int64, device=DEV), *data)
        ring = DevicePrioritizedRing(cap, device=DEV) if prioritized else ReplayRing(cap, device=DEV)
        ring.push(*data)
        seq.append(Learner(TD3(TD3Config(), device=DEV, seed=j), ring, B, graphs=True, warm_pairs=1, fused=True))
    grouped = PopulationLearner([TD3(TD3Config(), device=DEV, seed=j) for j in range(S)],
                                [pop.member(j) for j in range(S)], B, warm_pairs=1)

    def run_grouped(p):
        grouped.run(2 * p)

    def run_seq(p):
        for _ in range(p):
            for lr in seq:
                lr.run(2)

    for fn in (run_grouped, run_seq):  # warm-up pair, capture, a few replays
        fn(4)
    assert grouped.graph is not None and all(lr.graph is not None for lr in seq)
    g, s = [], []
    for _ in range(repeats):
        g.append(_timed(run_grouped, max(50, pairs // max(1, S // 8))))
        s.append(_timed(run_seq, max(5, pairs // S)))
    rec = {"members": S, "batch": B, "prioritized": prioritized, "grouped_ms_per_pair": g, "sequential_ms_per_pair": s,
           "grouped_median": statistics.median(g), "sequential_median": statistics.median(s)}
    rec["sequential_over_grouped"] = rec["sequential_median"] / rec["grouped_median"]
    rec["grouped_ms_per_member_update"] = rec["grouped_median"] / (2 * S)
    return rec


def push_bench(S, pushes, repeats, arenas=20, cap=8192):
    """ms per ragged push of S x arenas rows (one training step's transitions), with and without priorities."""
    rings = {"with_priorities": PopulationPrioritizedRing(S, cap, device=DEV),
             "without_priorities": PopulationRing(S, cap, device=DEV)}
    n = S * arenas
    member = torch.arange(n, device=DEV) // arenas
    data = _fill(n, 7)

    def run(ring):
        return lambda k: [ring.push(member, *data) for _ in range(k)]

    rec = {"members": S, "rows_per_push": n, "pushes_per_timing": pushes}
    for ring in rings.values():  # warm-up past one wrap of the ring
        run(ring)(cap // arenas + 8)
    times = {k: [] for k in rings}
    for _ in range(repeats):
        for k, ring in rings.items():
            times[k].append(_timed(run(ring), pushes))
    for k, t in times.items():
        rec[k + "_ms_per_push"] = t
        rec[k + "_median"] = statistics.median(t)
    rec["priorities_over_plain"] = rec["with_priorities_median"] / rec["without_priorities_median"]
    return rec


def round_bench(S, arenas=20):
    cfg = TD3Config(max_steps=250, use_self_play=False, curriculum_name="noise_study")
    _, st = train_population([(cfg, 100 + j) for j in range(S)], n_arenas=arenas, rounds=2, device=DEV, timing=True)
    pop_round = st[0]["round_time"][1]
    seq_collect = seq_update = 0.0
    for j in range(S):
        _, s1 = train(n_arenas=arenas, rounds=2, cfg=cfg, device=DEV, seed=100 + j, timing=True)
        seq_collect += s1["round_time"][1][0]
        seq_update += s1["round_time"][1][1]
        updates = s1["updates_per_round"]
    rec = {"members": S, "arenas_per_member": arenas, "steps": cfg.max_steps, "updates_per_round": updates,
           "population_updates_per_round": st[0]["updates_per_round"],
           "population_round_s": {"collect": pop_round[0], "update": pop_round[1], "total": sum(pop_round)},
           "sequential_rounds_s": {"collect": seq_collect, "update": seq_update, "total": seq_collect + seq_update}}
    rec["sequential_over_population"] = rec["sequential_rounds_s"]["total"] / rec["population_round_s"]["total"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,32,64")
    ap.add_argument("--round-sizes", default="8,32")
    ap.add_argument("--pairs", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--prioritized", action="store_true",
                    help="the prioritized-replay leg: grouped against sequential update pairs, and the ragged push "
                         "with and without priorities")
    ap.add_argument("--pushes", type=int, default=300)
    ap.add_argument("--out", default="population_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("population_bench needs the GPU (no CPU fallback)")
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "pairs_per_timing": args.pairs, "learner": [],
           "round": [], "push": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def record(key, rec):  # the file is rewritten after every measurement
        out[key].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    if args.prioritized:
        for S in (int(x) for x in args.sizes.split(",") if x):
            record("learner", learner_bench(S, args.pairs, args.repeats, prioritized=True))
            record("push", push_bench(S, args.pushes, args.repeats))
        return
    for S in (int(x) for x in args.sizes.split(",") if x):
        record("learner", learner_bench(S, args.pairs, args.repeats))
    for S in (int(x) for x in args.round_sizes.split(",") if x):
        record("round", round_bench(S))


if __name__ == "__main__":
    main()

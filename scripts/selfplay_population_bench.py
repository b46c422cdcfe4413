#!/usr/bin/env python3
"""Population self-play on the wide policy bank: three measurements, one JSON (profiles/r18).

(a) act     one acting call over 65 536 rows on 40 policies (scripts/act_bench.py's load): ``hkl_act`` (a 40-slot
            bank) beside ``hkl_act_wide`` (the same 40 actors in a 65-slot bank, which takes the wide path).
(b) select  S = 8 / 32 / 64 members x 20 arenas, P(self-play) = 0.3, every pool full (12 snapshots): ONE
            ``PopulationOpponentMix.select`` beside S ``OpponentMix(sampling="arena").select`` calls in turn, each
            over its member's 20 arenas -- what a population had to do before.  Also the acting kernel's tiles per
            call (counted from the returned policy tensor) and the bytes they read, computed from the shapes: a tile
            reads its policy's forward fragments (fc1, fc2, fc3 operand packs) and biases.
(c) round   one training round (20 arenas x 250 steps + 640 updates per member) of ``train_population(self_play=
            "arena")`` beside the same members as separate ``train(self_play_sampling="arena")`` runs in turn: the
            second of two rounds each, so that every pool holds a snapshot and the self-play share (0.3) is played.

Legs alternate inside every repetition, each figure is the median of ``--repeats`` (5) repetitions, all in one process
on one stream: measured, one session.  (a) is timed by HIP events around one call, (b) and (c) by the host clock around
work that ends in a device synchronise, because their cost is mostly launches and host work.

    python scripts/selfplay_population_bench.py [--parts a,b,c] [--out profiles/r18/selfplay_population_bench.json]
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

from hockey_amd.evaluate import Actor  # noqa: E402
from hockey_amd.opponents import CURRICULA, OpponentMix, PopulationOpponentMix  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402
from hockey_amd.td3 import TD3Config  # noqa: E402

DEV = "cuda:0"
TABLE = [(1.0, 0.35, 0.35, 0.3)]
# floats one acting tile reads of its policy: the fc1 / fc2 / fc3 forward fragments of the operand pack
# (csrc/hkl_mlp.h kF1, kFp, kFo) and the three biases from the parameter block
TILE_FLOATS = 16 * 64 * 8 + 16 * 16 * 64 * 4 + 16 * 64 * 4 + 256 + 256 + 4


def _median(xs):
    return statistics.median(xs)


def act_bench(rows, calls, repeats):
    torch.manual_seed(0)
    actors = [Actor().to(DEV).eval() for _ in range(40)]
    narrow, wide = PolicyBank(40, DEV), PolicyBank(65, DEV, wide=True)
    narrow.replace_many(range(40), actors)
    wide.replace_many(range(40), actors)
    obs = torch.randn(rows, 18, device=DEV)
    policy = torch.randint(0, 40, (rows,), device=DEV, dtype=torch.int32)
    outs = {"hkl_act": torch.zeros((rows, 8), device=DEV), "hkl_act_wide": torch.zeros((rows, 8), device=DEV)}
    legs = {"hkl_act": lambda: narrow.act(obs, policy, out=outs["hkl_act"], out_col=4, backend="hip"),
            "hkl_act_wide": lambda: wide.act(obs, policy, out=outs["hkl_act_wide"], out_col=4, backend="hip")}
    stream = torch.cuda.current_stream()
    for _ in range(5):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    assert torch.equal(outs["hkl_act"], outs["hkl_act_wide"])  # the same bits, at the size that is timed
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        ev = {k: [] for k in legs}
        for _ in range(calls):
            for k, fn in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                fn()
                t1.record(stream)
                ev[k].append((t0, t1))
        torch.cuda.synchronize()
        for k in legs:
            ms[k].append(_median([a.elapsed_time(b) for a, b in ev[k]]))
    rec = {"rows": rows, "policies": 40, "calls_per_repeat": calls,
           "ms_per_call": ms, "median_ms": {k: _median(v) for k, v in ms.items()}}
    rec["wide_over_narrow"] = rec["median_ms"]["hkl_act_wide"] / rec["median_ms"]["hkl_act"]
    return rec


def select_bench(S, calls, repeats, n=20, pool=12):
    torch.manual_seed(S)
    cfg = TD3Config(use_self_play=True, self_play_interval=250, self_play_pool_size=pool)
    actors = [Actor().to(DEV).eval() for _ in range(pool)]
    pop = PopulationOpponentMix([cfg] * S, list(range(S)), n, DEV, "arena", backend="hip", curriculum=TABLE)
    for i in range(pool):  # every pool full; S snapshots per replace_many
        pop.snapshot(list(range(S)), [actors[(j + i) % pool] for j in range(S)])
    singles = []
    for j in range(S):
        m = OpponentMix(n, TABLE, True, 250, pool, DEV, j, sampling="arena", backend="hip")
        for a in actors:
            m.pool.add_snapshot(a)
        singles.append(m)
    obs2 = torch.randn(S * n, 18, device=DEV)
    rows = [obs2[j * n:(j + 1) * n] for j in range(S)]
    act8 = torch.zeros((S * n, 8), device=DEV)
    outs = [act8[j * n:(j + 1) * n] for j in range(S)]

    def one():
        pop.select(obs2, act8)

    def per_member():
        for m, o, out in zip(singles, rows, outs):
            m.select(o, out)

    legs = {"population_select": one, "per_member_selects": per_member}
    for _ in range(5):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
    tiles, acting = [], []
    for _ in range(20):  # the acting kernel's work per call: tiles = sum over policies of ceil(rows / 64)
        _, _, policy = pop.select(obs2, act8)
        p = policy[policy >= 0].long()
        counts = torch.bincount(p, minlength=pop.bank.capacity)
        tiles.append(int(((counts + 63) // 64).sum()))
        acting.append(int(p.numel()))
    pop.reset_stats()
    for m in singles:
        m.reset_stats()
    rec = {"members": S, "arenas_per_member": n, "p_self": TABLE[0][3], "pool": pool, "bank_slots": pop.bank.capacity,
           "calls_per_repeat": calls, "ms_per_step": ms, "median_ms": {k: _median(v) for k, v in ms.items()},
           "acting_rows_per_call_mean": statistics.mean(acting), "tiles_per_call_mean": statistics.mean(tiles),
           "bytes_per_tile": 4 * TILE_FLOATS,
           "acting_kernel_bytes_per_call_mean": 4 * TILE_FLOATS * statistics.mean(tiles)}
    rec["per_member_over_population"] = rec["median_ms"]["per_member_selects"] / rec["median_ms"]["population_select"]
    return rec


def round_bench(S, repeats, arenas=20):
    from hockey_amd.population import train_population
    from hockey_amd.td3 import train

    CURRICULA["selfplay_bench"] = TABLE
    cfg = TD3Config(max_steps=250, use_self_play=True, curriculum_name="selfplay_bench", self_play_interval=arenas,
                    self_play_pool_size=12)
    pop, seq = [], []
    for _ in range(repeats):
        _, st = train_population([(cfg, 100 + j) for j in range(S)], n_arenas=arenas, rounds=2, device=DEV, timing=True,
                                 self_play="arena")
        pop.append(sum(st[0]["round_time"][1]))
        pools = [s["pool_size"] for s in st]
        played = sum(s["opponents"][1]["self_play"] for s in st)
        total = 0.0
        for j in range(S):
            _, s1 = train(n_arenas=arenas, rounds=2, cfg=cfg, device=DEV, seed=100 + j, timing=True,
                          self_play_sampling="arena")
            total += sum(s1["round_time"][1])
            updates = s1["updates_per_round"]
        seq.append(total)
    rec = {"members": S, "arenas_per_member": arenas, "steps": cfg.max_steps, "updates_per_round": updates,
           "population_updates_per_round": st[0]["updates_per_round"], "pool_sizes_member0": pools[0],
           "self_play_arena_steps_round2": played, "population_round_s": pop, "sequential_rounds_s": seq,
           "population_median_s": _median(pop), "sequential_median_s": _median(seq)}
    rec["sequential_over_population"] = rec["sequential_median_s"] / rec["population_median_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--sizes", default="8,32,64")
    ap.add_argument("--round-sizes", default="8,32")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--round-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "selfplay_population_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("selfplay_population_bench needs the GPU (no CPU fallback)")
    out = {"what": "medians of alternated legs in one process: measured, one session",
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "act": [], "select": [], "round": []}
    if os.path.exists(args.out):  # parts measured by an earlier call of the same session are kept
        with open(args.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k in ("act", "select", "round")})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def record(key, rec):  # the file is rewritten after every measurement
        out[key].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    parts = args.parts.split(",")
    if "a" in parts:
        record("act", act_bench(args.rows, args.calls, args.repeats))
    if "b" in parts:
        for S in (int(x) for x in args.sizes.split(",") if x):
            record("select", select_bench(S, args.calls, args.repeats))
    if "c" in parts:
        for S in (int(x) for x in args.round_sizes.split(",") if x):
            record("round", round_bench(S, args.round_repeats))


if __name__ == "__main__":
    main()

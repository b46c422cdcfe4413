#!/usr/bin/env python3
"""Two side measurements behind DESIGN.md §5's account of the seeded reset, at 65 536 arenas on one MI355X:

  wrapper   where the host time of VecHockeyEnv.reset_seeded goes: wall-clock medians of the whole call beside
            reset(), of its pieces (seed check, one_starts mirror, its upload) and of the raw ABI calls, each piece
            ending in a device synchronise  -> wrapper_split.json
  sides     50 hk_step launches of strong-vs-strong fused bots after a reset, HIP events: the puck side dealt per
            arena alternately (the reference's episode parity), one side per round, half and half, and the Philox
            reset  -> side_mix.json

    python scripts/seeded_reset_split.py [--out-dir profiles/r13]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))

N_ARENAS = 65536


def wrapper(np, torch, out_dir):
    from hockey_amd import _native as N
    from hockey_amd.vec_env import VecHockeyEnv

    n, dev = N_ARENAS, torch.device("cuda:0")
    env = VecHockeyEnv(n, device=dev)
    L, ctx = env.L, env._ctx

    def med(fn, reps=30):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    one = (np.arange(n, dtype=np.int64) % 2) == 1
    seeds = torch.arange(1, n + 1, device=dev)
    out = {
        "reset_philox_wrapper_ms": med(lambda: env.reset()),
        "reset_seeded_wrapper_ms": med(lambda: env.reset_seeded(seeds, one_starting=one)),
        "reset_seeded_wrapper_no_side_ms": med(lambda: env.reset_seeded(seeds)),
        "seed_tensor_check_ms": med(lambda: env._seed_tensor(seeds)),
        "mirror_ms": med(lambda: env._mirror_one_starts(None, one)),
        "one_upload_ms": med(lambda: torch.as_tensor(env.one_starts.astype(np.uint8), device=dev)),
        "arange_ms": med(lambda: (np.arange(n, 2 * n, dtype=np.int64), torch.arange(1, n + 1, device=dev))),
        "raw_hk_reset_seeded_ms": med(lambda: L.hk_reset_seeded(ctx, None, N.ptr(seeds), None, None, env._stream())),
        "raw_hk_reset_ms": med(lambda: L.hk_reset(ctx, None, None, None, None, env._stream())),
        "observe_ms": med(lambda: env.observe()),
        "clone_obs_ms": med(lambda: [t.clone() for t in (env.obs_buf, env.obs2_buf)]),
    }
    env.close()
    _write(out_dir, "wrapper_split.json", out)


def sides(np, torch, out_dir, steps=50, reps=12):
    from hockey_amd.vec_env import VecHockeyEnv

    n, dev = N_ARENAS, torch.device("cuda:0")
    env = VecHockeyEnv(n, device=dev, policies=("strong", "strong"))
    stream = torch.cuda.current_stream(dev)
    alt = (np.arange(n) % 2) == 1
    half = np.arange(n) >= n // 2
    times = {"seeded_alternating": [], "seeded_one_side": [], "philox_one_side": [], "seeded_half_split": []}

    def run(kind, r):
        seeds = torch.arange(1 + r * n, 1 + (r + 1) * n, device=dev)
        if kind == "seeded_alternating":
            env.reset_seeded(seeds, one_starting=alt)
        elif kind == "seeded_one_side":
            env.reset_seeded(seeds, one_starting=bool(r % 2))
        elif kind == "seeded_half_split":
            env.reset_seeded(seeds, one_starting=half)
        else:
            env.reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(steps):
            env.step(None)
        t1.record(stream)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    for r in range(reps + 2):  # the legs alternate; the first two rounds warm up
        for kind in times:
            ms = run(kind, r)
            if r >= 2:
                times[kind].append(ms)
    env.close()
    _write(out_dir, "side_mix.json", {k: {"ms_median_50_steps": statistics.median(v), "ms_min": min(v),
                                          "ms_max": max(v)} for k, v in times.items()})


def _write(out_dir, name, out):
    print(json.dumps(out, indent=1))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name), "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r13"))
    args = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "seeded_reset_split measures on the GPU only"
    wrapper(np, torch, args.out_dir)
    sides(np, torch, args.out_dir)
    return 0


if __name__ == "__main__":
    sys.exit(main())

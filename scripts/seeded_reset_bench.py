#!/usr/bin/env python3
"""Cost of a seeded reset at 65 536 arenas: the device draw (hk_reset_seeded) beside the Philox reset (hk_reset) and
beside the host path it replaces (numpy draws, upload, hk_reset), and what that does to the collection rate of
hockey_amd.td3.train.

Legs, each in a child process of its own under `timeout`; a leg that fails ends the run (nothing more is started on
the GPU):
  reset         hk_reset_seeded, hk_seeded_params and the Philox hk_reset alternate on one stream, each launch timed
                by a pair of HIP events after warm-up: medians of >= 20 launches, ms per call.  Then the host path,
                wall seconds ending in a device synchronise, split into evaluate.reset_params (the numpy draws),
                the upload and hk_reset: median of --host-reps.
  train_<how>   rounds of train(reset=<how>) for how = seeded (device draw), seeded_host (host draw), device (Philox)
                on bench.py's C5 collection shape (65 536 arenas x 50 steps, stage-3 opponent mix), no learner
                updates, timing=True: env-steps/s of the collection of every round after the first.  The seeded and
                device legs run in two processes each, alternating; the summary pools a leg's rounds and lists each
                process's median beside it.

    python scripts/seeded_reset_bench.py [--launches 30] [--out profiles/r13/seeded_reset_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))

N_ARENAS = 65536
TRAIN_STEPS = 50
TRAIN_ROUNDS = 4  # the first is left out (an empty self-play pool, first launches)
TRAIN_LEGS = ("seeded", "seeded_host", "device")
# child processes in this order: seeded and device run twice, alternating, so that the spread between two processes of
# the same leg stands beside the difference between the legs
TRAIN_ORDER = ("seeded", "device", "seeded_host", "device", "seeded")
LEG_TIMEOUT_S = 420
TAG = "SEEDED_RESET_BENCH "


def summary(ms):
    ms = sorted(ms)
    return {"ms_median": statistics.median(ms), "ms_min": ms[0], "ms_max": ms[-1]}


def leg_reset(launches, host_reps, warmup=5):
    import numpy as np
    import torch

    from hockey_amd import _native as N
    from hockey_amd.evaluate import reset_params
    from hockey_amd.vec_env import VecHockeyEnv

    assert torch.cuda.is_available(), "seeded_reset_bench measures on the GPU only"
    dev = torch.device("cuda:0")
    env = VecHockeyEnv(N_ARENAS, device=dev)
    stream = torch.cuda.current_stream(dev)
    seeds = torch.arange(1, N_ARENAS + 1, device=dev, dtype=torch.int64)
    params = torch.empty((N_ARENAS, 6), dtype=torch.float32, device=dev)
    L, ctx, st = env.L, env._ctx, env._stream()

    calls = {
        "hk_reset_seeded": lambda: N.check(L.hk_reset_seeded(ctx, None, N.ptr(seeds), None, None, st), "reset_seeded"),
        "hk_seeded_params": lambda: N.check(L.hk_seeded_params(ctx, N.ptr(seeds), None, N.ptr(params), None, st),
                                            "seeded_params"),
        "hk_reset_philox": lambda: N.check(L.hk_reset(ctx, None, None, None, None, st), "reset"),
    }

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        return t0, t1

    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize(dev)
    ev = {k: [] for k in calls}
    for _ in range(launches):
        for k, fn in calls.items():
            ev[k].append(timed(fn))
    torch.cuda.synchronize(dev)
    res = {"leg": "reset", "arenas": N_ARENAS, "launches": launches, "device": torch.cuda.get_device_name(dev)}
    for k, pairs in ev.items():
        res[k] = summary([x.elapsed_time(y) for x, y in pairs])
    res["seeded_over_philox"] = res["hk_reset_seeded"]["ms_median"] / res["hk_reset_philox"]["ms_median"]

    host = {"draw_s": [], "upload_s": [], "reset_s": [], "total_s": []}
    for r in range(host_reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        p, _, _ = reset_params(N_ARENAS, 1 + r * N_ARENAS)
        t1 = time.perf_counter()
        pt = torch.as_tensor(p, device=dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        N.check(L.hk_reset(ctx, None, N.ptr(pt), None, None, st), "reset")
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        for k, v in zip(host, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
            host[k].append(v)
    res["host_path"] = {k: statistics.median(v) for k, v in host.items()}
    res["host_path"]["reps"] = host_reps
    # the device draw of the last host batch equals it (the comparison is of equal work)
    got, _ = env.seeded_params(np.arange(N_ARENAS, dtype=np.int64) + 1 + (host_reps - 1) * N_ARENAS,
                               one_starting=(np.arange(N_ARENAS) % 2) == 1)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), p.view(np.uint32))
    res["host_over_device"] = res["host_path"]["total_s"] * 1e3 / res["hk_reset_seeded"]["ms_median"]
    print(TAG + json.dumps(res), flush=True)
    env.close()


def leg_train(how):
    import torch

    from hockey_amd.td3 import TD3Config, train

    assert torch.cuda.is_available(), "seeded_reset_bench measures on the GPU only"
    dev = "cuda:0"
    table = [(1.0, 0.35, 0.35, 0.30)]  # bench.py time_c5: stage-3's last curriculum row
    kw = dict(device=dev, curriculum=table, self_play_interval=N_ARENAS, reset=how, updates_per_round=0)
    train(n_arenas=N_ARENAS, rounds=2, cfg=TD3Config(max_steps=5, start_steps=0), **kw)  # warm-up
    _, st = train(n_arenas=N_ARENAS, rounds=TRAIN_ROUNDS, cfg=TD3Config(max_steps=TRAIN_STEPS, start_steps=0),
                  timing=True, **kw)
    collect = [c for c, _ in st["round_time"][1:]]
    rates = sorted(N_ARENAS * TRAIN_STEPS / c for c in collect)
    res = {"leg": "train_" + how, "reset": how, "arenas": N_ARENAS, "steps": TRAIN_STEPS, "rounds_timed": len(collect),
           "collect_s": collect, "env_steps_per_s_median": statistics.median(rates), "env_steps_per_s_min": rates[0],
           "env_steps_per_s_max": rates[-1], "device": torch.cuda.get_device_name(0)}
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["reset"] + ["train_" + h for h in TRAIN_LEGS])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "seeded_reset_bench.json"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches must be at least 20")
    if args.leg == "reset":
        leg_reset(args.launches, args.host_reps)
        return 0
    if args.leg:
        leg_train(args.leg[len("train_"):])
        return 0
    legs = []
    for name in ["reset"] + ["train_" + h for h in TRAIN_ORDER]:
        r = subprocess.run(["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                            "--leg", name, "--launches", str(args.launches), "--host-reps", str(args.host_reps)],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not line:
            print(f"leg {name} failed ({r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            return 1
        legs.append(json.loads(line[-1][len(TAG):]))
        print(line[-1], flush=True)
    collect = {}
    for how in TRAIN_LEGS:
        procs = [leg for leg in legs if leg["leg"] == "train_" + how]
        rates = [N_ARENAS * TRAIN_STEPS / c for leg in procs for c in leg["collect_s"]]
        collect[how] = {"env_steps_per_s_median": statistics.median(rates), "env_steps_per_s_min": min(rates),
                        "env_steps_per_s_max": max(rates),
                        "per_process_median": [leg["env_steps_per_s_median"] for leg in procs]}
    out = {"what": "seeded resets at 65 536 arenas: HIP-event medians of the device calls, wall seconds of the host "
                   "path, and train()'s collection rate per reset mode; one session, one MI355X",
           "legs": legs, "collect": collect,
           "collect_seeded_over_seeded_host": collect["seeded"]["env_steps_per_s_median"] /
           collect["seeded_host"]["env_steps_per_s_median"],
           "collect_seeded_over_device": collect["seeded"]["env_steps_per_s_median"] /
           collect["device"]["env_steps_per_s_median"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Time of one value call over 65 536 rows -- hkl_value (ValueFn backend="hip") beside the eager PyTorch path it
replaces -- and of one ShootingPlanner.act at M = 1 024 arenas, K = 64 branches, H = 8 steps.

Legs of the value call (one Actor and one TwinQ with the same weights on both sides, the same rows):
  hip_v      hkl_value, V mode: actor + both critics + min in one launch, the action in registers
  torch_v    Actor.forward, TwinQ.forward (unscale, cat, two MLPs), torch.minimum
  hip_q      hkl_value, Q mode on given actions (qmin)
  torch_q    TwinQ.forward + torch.minimum

The planner call, and beside it its parts run on their own in the same order on the same workspace:
  planner_act      ShootingPlanner.act() as a whole (base action, candidates, fork, rollout, value, argmax)
  planner_fork     the M * K arena copies (VecHockeyEnv.fork from the live env)
  planner_rollout  hk_rollout of H steps over the M * K workspace arenas, player 2 a fused strong bot
  planner_value    hk_observe + hkl_value (V mode) on the M * K rows
  planner_rest_ms  planner_act - (fork + rollout + value), from the medians

One process, one stream; every leg is timed by a pair of HIP events after warm-up and the medians of >= 20
repetitions are reported (the legs alternate inside a repetition), with the ratio of each torch leg to its hip leg and
the fp32 FLOP rate of the hip legs (2 FLOP per multiply-add of the three / two networks).

    python scripts/value_bench.py [--rows 65536] [--launches 30] [--out profiles/r14/value_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))

FLOP_ACTOR = 2 * (18 * 256 + 256 * 256 + 256 * 4)
FLOP_CRITIC = 2 * (22 * 256 + 256 * 256 + 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arenas", type=int, default=1024)
    ap.add_argument("--branches", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "value_bench.json"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches must be at least 20")

    import torch

    from hockey_amd import _native as N
    from hockey_amd.evaluate import Actor
    from hockey_amd.planner import ShootingPlanner
    from hockey_amd.td3 import TwinQ
    from hockey_amd.value import ValueFn
    from hockey_amd.vec_env import VecHockeyEnv

    assert torch.cuda.is_available(), "value_bench measures on the GPU only"
    dev = torch.device("cuda:0")
    n = args.rows
    torch.manual_seed(0)
    actor, critic = Actor().to(dev).eval(), TwinQ().to(dev).eval()
    vf = ValueFn((actor, critic), dev)
    obs = torch.randn(n, 18, device=dev)
    act = torch.rand(n, 4, device=dev) * 2 - 1
    stream = torch.cuda.current_stream(dev)

    def torch_v():
        with torch.no_grad():
            return torch.minimum(*critic(obs, actor(obs)))

    def torch_q():
        with torch.no_grad():
            return torch.minimum(*critic(obs, act))

    # the planner and its parts
    M, K, H = args.arenas, args.branches, args.horizon
    env = VecHockeyEnv(M, device=dev, policies=("external", "strong"), seed=1)
    env.reset()
    for _ in range(10):
        env.step(torch.rand(M, 8, device=dev) * 2 - 1)
    planner = ShootingPlanner(env, vf, branches=K, horizon=H, opponent="basic_strong", seed=0)
    la, ws = planner.la, planner.la.ws
    src = torch.arange(M, device=dev).repeat_interleave(K)
    io = N.StepIO()
    io.actions, io.opp_inc = la._act.data_ptr(), None
    io.reward, io.done = la._rew.data_ptr(), la._done.data_ptr()

    legs = {"hip_v": lambda: vf.v(obs, backend="hip"), "torch_v": torch_v,
            "hip_q": lambda: vf.qmin(obs, act, backend="hip"), "torch_q": torch_q,
            "planner_act": planner.act,
            "planner_fork": lambda: ws.fork(src, None, source=env),
            "planner_rollout": lambda: ws.rollout_raw(H, io),
            "planner_value": lambda: vf.v(ws.observe()[0])}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        return t0, t1

    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize(dev)
    ev = {k: [] for k in legs}
    for _ in range(args.launches):  # the legs alternate, so that drift of the shared machine touches all alike
        for k, fn in legs.items():
            ev[k].append(timed(fn))
        torch.cuda.synchronize(dev)
    flop = {"hip_v": (FLOP_ACTOR + 2 * FLOP_CRITIC) * n, "hip_q": 2 * FLOP_CRITIC * n}
    res = {"what": "one value call over `rows` rows and one ShootingPlanner.act: medians of HIP-event timings in one "
                   "process", "rows": n, "launches": args.launches, "warmup": args.warmup,
           "planner": {"arenas": M, "branches": K, "horizon": H, "opponent": "basic_strong"},
           "device": torch.cuda.get_device_name(dev), "legs": {}}
    for k, pairs in ev.items():
        ms = sorted(a.elapsed_time(b) for a, b in pairs)
        med = statistics.median(ms)
        res["legs"][k] = {"ms_median": med, "ms_min": ms[0], "ms_max": ms[-1]}
        if k in flop:
            res["legs"][k]["flop_per_call"] = flop[k]
            res["legs"][k]["tflops_fp32"] = flop[k] / (med * 1e-3) / 1e12
    m = {k: v["ms_median"] for k, v in res["legs"].items()}
    for mode in ("v", "q"):
        res[f"torch_over_hip_{mode}"] = m[f"torch_{mode}"] / m[f"hip_{mode}"]
    res["planner_rest_ms"] = m["planner_act"] - (m["planner_fork"] + m["planner_rollout"] + m["planner_value"])
    print("VALUE_BENCH " + json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    planner.close()
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

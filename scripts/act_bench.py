#!/usr/bin/env python3
"""Time of one acting call over 65 536 rows: hkl_act (PolicyBank backend="hip") beside the PyTorch paths it replaces.

Legs (K = policies in the bank, every row assigned uniformly at random):
  hip_k1     hkl_act, policy = NULL (one actor, nothing grouped)
  torch_k1   the eager forward of one Actor over every row (PolicyOpponent / OpponentMix sampling="step")
  hip_k40    hkl_act, 40 policies: histogram + scan + scatter + the grouped forward
  torch_k40  one masked eager forward per slot (PolicyBank backend="torch"): 40 forwards over every row

One process, one stream; every launch is timed by a pair of HIP events after warm-up and the medians of >= 20
launches are reported, with the ratio of each torch leg to its hip leg and the fp32 FLOP rate of the hip legs
(2 x (18 x 256 + 256 x 256 + 256 x 4) FLOP per row).

    python scripts/act_bench.py [--rows 65536] [--launches 30] [--out profiles/r09/act_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))

FLOP_PER_ROW = 2 * (18 * 256 + 256 * 256 + 256 * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "act_bench.json"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches must be at least 20")

    import torch

    from hockey_amd.evaluate import Actor
    from hockey_amd.policy_bank import PolicyBank

    assert torch.cuda.is_available(), "act_bench measures on the GPU only"
    dev = torch.device("cuda:0")
    n = args.rows
    torch.manual_seed(0)
    actors = [Actor().to(dev).eval() for _ in range(40)]
    bank1, bank40 = PolicyBank(1, dev), PolicyBank(40, dev)
    bank1.add(actors[0])
    for a in actors:
        bank40.add(a)
    obs = torch.randn(n, 18, device=dev)
    policy = torch.randint(0, 40, (n,), device=dev, dtype=torch.int32)
    out = torch.zeros((n, 8), device=dev)
    stream = torch.cuda.current_stream(dev)

    def torch_k1():
        with torch.no_grad():
            out[:, 4:] = actors[0](obs)

    legs = {"hip_k1": lambda: bank1.act(obs, out=out, out_col=4, backend="hip"),
            "torch_k1": torch_k1,
            "hip_k40": lambda: bank40.act(obs, policy, out=out, out_col=4, backend="hip"),
            "torch_k40": lambda: bank40.act(obs, policy, out=out, out_col=4, backend="torch")}

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
    res = {"what": "one acting call over `rows` rows: medians of HIP-event timings in one process",
           "rows": n, "launches": args.launches, "warmup": args.warmup, "flop_per_call": FLOP_PER_ROW * n,
           "device": torch.cuda.get_device_name(dev), "legs": {}}
    for k, pairs in ev.items():
        ms = sorted(a.elapsed_time(b) for a, b in pairs)
        med = statistics.median(ms)
        res["legs"][k] = {"ms_median": med, "ms_min": ms[0], "ms_max": ms[-1]}
        if k.startswith("hip"):
            res["legs"][k]["tflops_fp32"] = FLOP_PER_ROW * n / (med * 1e-3) / 1e12
    for K in ("k1", "k40"):
        res[f"torch_over_hip_{K}"] = res["legs"][f"torch_{K}"]["ms_median"] / res["legs"][f"hip_{K}"]["ms_median"]
    print("ACT_BENCH " + json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

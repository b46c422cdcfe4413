"""Time per fused learner update with uniform sampling, torch prioritized replay (PrioritizedRing: whole-ring PyTorch
ops) and device prioritized replay (DevicePrioritizedRing: the hkl_per_* kernels), and the per-step push cost of the
rings, at batch 16 384 on rings of 2^20 and 32 768 000 slots (C5: 65 536 arenas x 500 steps).

Each ring is filled through push (chunks of 65 536 transitions, one C5 step); the prioritized rings' weights then come
from 300 real updates, not from the all-1e8 initial state.  Timing: HIP events around K updates of Learner.run (the
production path: update pairs replayed as a HIP graph; --eager adds the kernel-by-kernel legs), the three legs
interleaved and repeated R times so that the run-to-run spread is visible; pushes likewise, on the full ring.
Writes one JSON record (default profiles/r07/per_bench.json) and rewrites it after every capacity.

Usage: python scripts/per_bench.py [--caps 1048576,32768000] [--batch 16384] [--updates 200] [--reps 5] [--eager]
                                   [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))
import torch  # noqa: E402

from hockey_amd.td3 import TD3, DevicePrioritizedRing, Learner, PrioritizedRing, ReplayRing, TD3Config  # noqa: E402

DEV = "cuda:0"
STEP = 65536  # transitions per push: one C5 collection step


def timed(fn):
    """Milliseconds of fn() between two HIP events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--caps", default="1048576,32768000")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pushes", type=int, default=50)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "per_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "per_bench.py measures on the GPU"
    rec = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "updates_per_window": a.updates,
           "repeats": a.reps, "push_transitions": STEP, "pushes_per_window": a.pushes, "unit": "ms", "capacity": {}}
    g = torch.Generator(device=DEV).manual_seed(0)
    chunk = (torch.randn(STEP, 18, device=DEV, generator=g), torch.rand(STEP, 4, device=DEV, generator=g) * 2 - 1,
             torch.randn(STEP, device=DEV, generator=g), torch.randn(STEP, 18, device=DEV, generator=g),
             (torch.rand(STEP, device=DEV, generator=g) < 0.01).float())
    for cap in (int(c) for c in a.caps.split(",")):
        n = min(STEP, cap)
        part = tuple(t[:n] for t in chunk)
        legs = {}
        for name, mk, cfg in (("uniform", ReplayRing, TD3Config()),
                              ("torch_per", PrioritizedRing, TD3Config(prioritized_replay=True)),
                              ("device_per", DevicePrioritizedRing, TD3Config(prioritized_replay=True))):
            ring = mk(cap, device=DEV) if mk is ReplayRing else mk(cap, device=DEV, beta=cfg.beta)
            for _ in range(-(-cap // n)):
                ring.push(*part)
            assert ring.size == cap
            modes = {"graph": True, "eager": False} if a.eager else {"graph": True}
            legs[name] = {"ring": ring,
                          "learner": {m: Learner(TD3(cfg, DEV, seed=0), ring, a.batch, graphs=gr, fused=True)
                                      for m, gr in modes.items()}}
            for lr in legs[name]["learner"].values():  # warm-up: every path, and the weights from real updates
                lr.run(300 // len(modes))
            torch.cuda.synchronize()
        out = {"update_ms": {}, "push_ms": {}}
        for mode in legs["uniform"]["learner"]:
            t = {k: [] for k in legs}
            for _ in range(a.reps):
                for k, leg in legs.items():
                    lr = leg["learner"][mode]
                    t[k].append(timed(lambda: lr.run(a.updates)) / a.updates)
            out["update_ms"][mode] = {k: spread(v) for k, v in t.items()}
        t = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, leg in legs.items():
                ring = leg["ring"]
                t[k].append(timed(lambda: [ring.push(*part) for _ in range(a.pushes)]) / a.pushes)
        out["push_ms"] = {k: spread(v) for k, v in t.items()}
        w = legs["device_per"]["ring"].w
        out["device_per_weights_left_init"] = int((w != 1e8).sum())
        u = out["update_ms"]["graph"]
        out["per_overhead_ms"] = {k: u[k]["median"] - u["uniform"]["median"] for k in ("torch_per", "device_per")}
        out["device_faster_than_torch_beyond_spread"] = u["device_per"]["max"] < u["torch_per"]["min"]
        rec["capacity"][str(cap)] = out
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({"capacity": cap, **{k: v for k, v in out.items()}}), flush=True)
        del legs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

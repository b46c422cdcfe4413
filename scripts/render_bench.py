#!/usr/bin/env python3
"""Throughput of the renderer (hkr_render) beside the store floor: a hipMemsetAsync of the same byte count.

Legs (frames x size x format):
  a  65 536 states at 84 x 84 INDEX      b  65 536 states at 84 x 84 RGB      c  1 024 states at 480 x 600 RGB

Each leg runs in a child process of its own under `timeout`; a leg that fails ends the run (nothing more is started
on the GPU).  Within a leg, render launches and memsets of the output buffer alternate on one stream, each timed by
a pair of HIP events after warm-up; the medians of >= 20 launches are reported as ms per launch and GB/s written.

    python scripts/render_bench.py [--launches 30] [--out profiles/r08/render_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hockey-env_amd"))

LEGS = {"a": (65536, 84, 84, "index"), "b": (65536, 84, 84, "rgb"), "c": (1024, 480, 600, "rgb")}
LEG_TIMEOUT_S = 240


def run_leg(name, launches, warmup=5):
    import numpy as np
    import torch

    from hockey_amd.constants import H, W
    from hockey_amd.render import render_states

    assert torch.cuda.is_available(), "render_bench measures on the GPU only"
    m, height, width, fmt = LEGS[name]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    st = np.zeros((m, 18), np.float32)  # bodies anywhere in the rink, rackets at any angle
    st[:, [0, 6, 12]] = rng.uniform(0.0, W, (m, 3))
    st[:, [1, 7, 13]] = rng.uniform(0.0, H, (m, 3))
    st[:, [2, 8]] = rng.uniform(-3.2, 3.2, (m, 2))
    state = torch.as_tensor(st, device=dev)
    out = torch.empty((m, height, width, 3) if fmt == "rgb" else (m, height, width), dtype=torch.uint8, device=dev)
    nbytes = out.numel()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemsetAsync.restype = ctypes.c_int
    stream = torch.cuda.current_stream(dev)

    def memset():
        rc = hip.hipMemsetAsync(ctypes.c_void_p(out.data_ptr()), 0, nbytes, ctypes.c_void_p(stream.cuda_stream))
        assert rc == 0, rc

    def render():
        render_states(state, None, height, width, fmt, out=out)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        return t0, t1

    for _ in range(warmup):
        render()
        memset()
    torch.cuda.synchronize(dev)
    ev = {"render": [], "memset": []}
    for _ in range(launches):
        ev["memset"].append(timed(memset))
        ev["render"].append(timed(render))
    torch.cuda.synchronize(dev)
    res = {"leg": name, "frames": m, "height": height, "width": width, "format": fmt, "bytes_written": nbytes,
           "launches": launches, "device": torch.cuda.get_device_name(dev)}
    for k, pairs in ev.items():
        ms = sorted(a.elapsed_time(b) for a, b in pairs)
        med = statistics.median(ms)
        res[k] = {"ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gb_per_s": nbytes / (med * 1e-3) / 1e9}
    res["render_over_memset_rate"] = res["render"]["gb_per_s"] / res["memset"]["gb_per_s"]
    print("RENDER_BENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "render_bench.json"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches must be at least 20")
    if args.leg:
        run_leg(args.leg, args.launches)
        return 0
    legs = []
    for name in sorted(LEGS):
        r = subprocess.run(["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                            "--leg", name, "--launches", str(args.launches)], capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RENDER_BENCH ")]
        if r.returncode != 0 or not line:
            print(f"leg {name} failed ({r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            return 1
        legs.append(json.loads(line[-1][len("RENDER_BENCH "):]))
        print(line[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "hkr_render beside hipMemsetAsync of the same bytes, medians of HIP-event timings",
                   "legs": legs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

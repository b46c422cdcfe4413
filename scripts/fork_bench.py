#!/usr/bin/env python3
"""Throughput of the exact arena copy (hk_copy_arenas) beside the copy floor: a device-to-device hipMemcpyAsync of
the same byte count in the same process.

Legs, each onto 65 536 consecutive destination arenas of a second context:
  a  identity: source arena e -> destination e
  b  replication: 1 024 source arenas x 64 (source e // 64 -> destination e), the lookahead shape

Each leg runs in a child process of its own under `timeout`; a leg that fails ends the run (nothing more is started
on the GPU).  Within a leg, forks and memcpys alternate on one stream, each timed by a pair of HIP events after
warm-up; the medians of >= 20 launches are reported as ms per launch and GB/s of arena bytes written (the copy reads
as many: in leg b mostly from L2).

    python scripts/fork_bench.py [--launches 30] [--out profiles/r11/fork_bench.json]
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

N_DST = 65536
LEGS = {"a": ("identity", N_DST), "b": ("1024 sources x 64", 1024)}
LEG_TIMEOUT_S = 240
HIP_MEMCPY_D2D = 3


def run_leg(name, launches, warmup=5):
    import torch

    from hockey_amd import snapshot as S
    from hockey_amd.vec_env import VecHockeyEnv

    assert torch.cuda.is_available(), "fork_bench measures on the GPU only"
    what, n_src = LEGS[name]
    dev = torch.device("cuda:0")
    src_env = VecHockeyEnv(n_src, device=dev, policies=("strong", "strong"), auto_reset=True)
    for _ in range(30):  # arenas with contacts and stored impulses (the copy is dense either way)
        src_env.step(None)
    dst_env = VecHockeyEnv(N_DST, device=dev)
    e = torch.arange(N_DST, device=dev, dtype=torch.int64)
    src = None if name == "a" else (e // (N_DST // n_src)).contiguous()
    nbytes = N_DST * sum(w * k for w, k in zip((4, 4, 8), S.library_layout()[:3]))
    nbytes += N_DST * S.library_layout()[3] * S.library_layout()[4] * 4
    a = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    stream = torch.cuda.current_stream(dev)

    def memcpy():
        rc = hip.hipMemcpyAsync(ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(a.data_ptr()), nbytes, HIP_MEMCPY_D2D,
                                ctypes.c_void_p(stream.cuda_stream))
        assert rc == 0, rc

    def fork():
        dst_env.fork(src, None, source=src_env, assume_valid=True)  # leg a: both lists NULL, the identity

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        return t0, t1

    for _ in range(warmup):
        fork()
        memcpy()
    torch.cuda.synchronize(dev)
    ev = {"fork": [], "memcpy": []}
    for _ in range(launches):
        ev["memcpy"].append(timed(memcpy))
        ev["fork"].append(timed(fork))
    torch.cuda.synchronize(dev)
    bad = int(dst_env.counters()[8])
    assert bad == 0, bad
    res = {"leg": name, "what": what, "destinations": N_DST, "sources": n_src, "bytes_written": nbytes,
           "bytes_per_arena": nbytes // N_DST, "launches": launches, "device": torch.cuda.get_device_name(dev)}
    for k, pairs in ev.items():
        ms = sorted(x.elapsed_time(y) for x, y in pairs)
        med = statistics.median(ms)
        res[k] = {"ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gb_per_s": nbytes / (med * 1e-3) / 1e9}
    res["fork_over_memcpy_rate"] = res["fork"]["gb_per_s"] / res["memcpy"]["gb_per_s"]
    print("FORK_BENCH " + json.dumps(res), flush=True)
    src_env.close()
    dst_env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "fork_bench.json"))
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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("FORK_BENCH ")]
        if r.returncode != 0 or not line:
            print(f"leg {name} failed ({r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            return 1
        legs.append(json.loads(line[-1][len("FORK_BENCH "):]))
        print(line[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "hk_copy_arenas beside hipMemcpyAsync (device to device) of the same bytes, medians of "
                           "HIP-event timings", "legs": legs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

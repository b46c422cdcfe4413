"""The seeded-reset case list and its numpy reference, shared by tests/test_seed_ref.py (csrc/hk_seed.h under g++)
and tests/test_gpu_seeded_reset.py (the gfx950 kernel behind hk_seeded_params / hk_reset_seeded).

* SEEDS: the edge seeds -- 0, 1, 2, the reference's 41/42/43, both sides of 2^31 and 2^32 (one entropy word
  against two), 2^53, both sides of 2^63 and 2^64 - 1 -- then 2 000 seeds from default_rng(0), half below 2^32 and
  half over the full 64 bits.
* cases(): every seed x the modes NORMAL, TRAIN_SHOOTING, TRAIN_DEFENSE x one_starts 0 / 1, 12 090 rows: not a
  multiple of 64, so the last wave of a lane-per-row kernel is partial.
* reference(rows): hockey_amd.placement.placement on np_random(seed) -- numpy's own SeedSequence, PCG64 and
  Generator.uniform -- computed once per process and returned read-only.
* host_probe(): tests/native/seed_probe_host.cpp, built with csrc's host flags.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hockey-env_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
LIBDIR = os.path.join(ROOT, "hockey-env_amd", "hockey_amd", "_lib")

N_RAW, N_DOUBLES = 8, 5  # seed_probe.h SP_RAW, SP_DOUBLES
CASE = np.dtype([("seed", np.uint64), ("mode", np.int32), ("one_starts", np.int32)])  # SpCase
PLACEMENT = np.dtype([("p6", np.float32, 6), ("max_t", np.int32), ("pad", np.int32)])  # SpPlacement
assert CASE.itemsize == 16 and PLACEMENT.itemsize == 32

EDGE_SEEDS = [0, 1, 2, 41, 42, 43, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**53, 2**63 - 1, 2**63, 2**64 - 1]
MODES = (0, 1, 2)  # NORMAL, TRAIN_SHOOTING, TRAIN_DEFENSE


def _seeds():
    rng = np.random.default_rng(0)
    low = rng.integers(0, 2**32, 1000, dtype=np.uint64)
    full = rng.integers(0, 2**64, 1000, dtype=np.uint64, endpoint=False)
    return np.concatenate([np.array(EDGE_SEEDS, np.uint64), low, full])


SEEDS = _seeds()
SEEDS.setflags(write=False)


@functools.lru_cache(None)
def cases():
    """All rows (CASE records), seed-major: seed x mode x one_starts."""
    rows = np.zeros(len(SEEDS) * len(MODES) * 2, CASE)
    rows["seed"] = np.repeat(SEEDS, len(MODES) * 2)
    rows["mode"] = np.tile(np.repeat(np.array(MODES, np.int32), 2), len(SEEDS))
    rows["one_starts"] = np.tile(np.array([0, 1], np.int32), len(SEEDS) * len(MODES))
    assert len(rows) % 64 != 0
    rows.setflags(write=False)
    return rows


@functools.lru_cache(None)
def reference():
    """PLACEMENT records of cases(): placement(mode, one_starts, np_random(seed)[0]), numpy all the way."""
    from hockey_amd.placement import np_random, placement

    rows = cases()
    out = np.zeros(len(rows), PLACEMENT)
    for i, r in enumerate(rows):
        rng, _ = np_random(int(r["seed"]))
        out["p6"][i], out["max_t"][i] = placement(int(r["mode"]), bool(r["one_starts"]), rng)
    out.setflags(write=False)
    return out


def mode_rows(mode):
    """(seeds uint64, one_starts uint8, params float32 [m,6], max_t int32) of the case rows of one mode."""
    rows, ref = cases(), reference()
    sel = rows["mode"] == int(mode)
    return (np.ascontiguousarray(rows["seed"][sel]), rows["one_starts"][sel].astype(np.uint8),
            np.ascontiguousarray(ref["p6"][sel]), np.ascontiguousarray(ref["max_t"][sel]))


@functools.lru_cache(None)
def host_probe():
    subprocess.check_call(["make", "-s", "-C", CSRC, "seed-probe-host"])
    L = ctypes.CDLL(os.path.join(LIBDIR, "libhockey_seed_probe_host.so"))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    for name in ("sp_state", "sp_raw", "sp_double"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [vp, i64, vp]
    L.sp_placement.restype = ctypes.c_int
    L.sp_placement.argtypes = [vp, i64, vp]
    return L


def host_flags():
    """csrc/Makefile's HOSTFLAGS (the project's host flags: no contraction, no fast-math)."""
    import re

    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^HOSTFLAGS = (.*)$", mk, flags=re.M).group(1).split()

"""A plain restatement of hkl_explore's law (include/hockey_explore.h) on learner_ref.philox4x32_10: Python integers
and float64 for the schedule, numpy for the draws.  Nothing here imports hockey_amd.explore.

Test infrastructure only.  tests/test_explore_ref.py holds this to a real ``TD3`` object (masks and scales) and the
package's torch backend to this; tests/test_gpu_explore.py holds the kernel to both.  A member is a dict with the keys
of ``member()``.
"""
import math

import numpy as np

from learner_ref import philox4x32_10

KEY_NOISE = int.from_bytes(b"explore", "big")  # HKL_EXPLORE_KEY_NOISE
KEY_RANDOM = int.from_bytes(b"random", "big")  # HKL_EXPLORE_KEY_RANDOM
MASK = (1 << 64) - 1


def member(seed=0, start_steps=0, max_total_steps=0, init_scale=0.2, min_scale=0.0, anneal="none", noise="gaussian",
           theta=0.15, dt=1.0):
    return dict(seed=seed, start_steps=start_steps, max_total_steps=max_total_steps, init_scale=init_scale,
                min_scale=min_scale, anneal=anneal, noise=noise, theta=theta, dt=dt)


def words(seed, purpose, n, calls):
    """[n, 4] uint32: the block of rows local = 0 .. n - 1 of a member at its call counter ``calls``."""
    ctr = np.zeros((n, 4), np.uint32)
    for i in range(n):
        ctr[i] = (i & 0xFFFFFFFF, i >> 32, calls & 0xFFFFFFFF, (calls >> 32) & 0xFFFFFFFF)
    return philox4x32_10(np.uint64((seed & MASK) ^ purpose), ctr)


def phase(total, count, n, start_steps):
    """(T0, T1, all_random, random [n] bool) of a member before a call."""
    t0 = max(int(total), 0)
    t1 = t0 + min(max(int(count), 0), n)
    all_random = t1 < start_steps
    return t0, t1, all_random, np.array([all_random or t0 + 1 + i < start_steps for i in range(n)], bool)


def scale64(mem, t1):
    """TD3.noise_scale() at total_steps = t1, as a Python float."""
    s = mem["init_scale"]
    if mem["anneal"] == "none" or mem["max_total_steps"] <= 0:
        return s
    progress = min(t1 / mem["max_total_steps"], 1.0)
    if mem["anneal"] == "linear":
        s = s * (1 - progress)
    elif mem["anneal"] == "exp":
        s = s * math.pow(0.1, progress)
    else:
        raise ValueError(mem["anneal"])
    return max(s, mem["min_scale"])


def uniform_pm1(w):
    """2 u - 1, u = (w >> 8) 2^-24: float64, and exactly representable in float32."""
    return 2.0 * ((w >> 8).astype(np.float64) * 2.0 ** -24) - 1.0


def normals(w, dtype=np.float64):
    """Box-Muller on the word pairs (x, y), (z, w): u1 = ((w >> 8) + 0.5) 2^-24, u2 = (w >> 8) 2^-24, (rad cos, rad sin)
    with rad = sqrt(-2 ln u1), angle = 2 pi u2 (the float32 2 pi, the kernel's constant).  ``dtype``: the precision the
    formula is evaluated in."""
    f = np.dtype(dtype).type
    z = np.zeros(w.shape, dtype)
    two_pi = f(np.float32(2.0 * np.pi))
    for p in range(2):
        u1 = ((w[:, 2 * p] >> 8).astype(dtype) + f(0.5)) * f(2.0 ** -24)
        u2 = (w[:, 2 * p + 1] >> 8).astype(dtype) * f(2.0 ** -24)
        rad = np.sqrt(f(-2.0) * np.log(u1))
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(two_pi * u2), rad * np.sin(two_pi * u2)
    return z


def call(members, n, total, calls, count, a, x=None, ext=None, z=None):
    """One call.  a, x, ext, z: [S n, 4]; z replaces the float32 normals (the kernel's z_out).  Every float32 product
    and sum is rounded on its own (numpy float32 arrays).  Returns out, x, z, scale [S] float32, random [S n], total,
    calls after the call."""
    S, f = len(members), np.float32
    a = np.asarray(a, f)
    out = np.full((S * n, 4), np.nan, f)
    xs = np.zeros((S * n, 4), f) if x is None else np.array(x, f)
    raw = np.zeros((S * n, 4), f)
    scale, rnd = np.zeros(S, f), np.zeros(S * n, bool)
    total, calls = [int(t) for t in total], [int(c) for c in calls]
    for m, mem in enumerate(members):
        r = slice(m * n, (m + 1) * n)
        t0, t1, all_random, rnd[r] = phase(total[m], count[m], n, mem["start_steps"])
        scale[m] = f(scale64(mem, t1))
        if not all_random:
            unit = np.zeros((n, 4), f)
            if mem["noise"] == "uniform":
                raw[r] = uniform_pm1(words(mem["seed"], KEY_NOISE, n, calls[m])).astype(f)
                unit = raw[r] * f(math.sqrt(3.0))
            elif mem["noise"] in ("gaussian", "ornstein-uhlenbeck"):
                raw[r] = normals(words(mem["seed"], KEY_NOISE, n, calls[m]), f) if z is None else np.asarray(z, f)[r]
                unit = raw[r]
                if mem["noise"] == "ornstein-uhlenbeck":
                    x0 = xs[r]
                    drift = (f(mem["theta"]) * (-x0)) * f(mem["dt"])
                    unit = (x0 + drift) + f(math.sqrt(mem["dt"])) * raw[r]
                    xs[r] = unit
            elif mem["noise"] == "external":
                unit = np.asarray(ext, f)[r]
            elif mem["noise"] != "none":
                raise ValueError(mem["noise"])
            v = a[r] + unit * scale[m]
            out[r] = np.where(v < -1, f(-1), np.where(v > 1, f(1), v))
        if rnd[r].any():
            u = uniform_pm1(words(mem["seed"], KEY_RANDOM, n, calls[m])).astype(f)
            out[r] = np.where(rnd[r][:, None], u, out[r])
        total[m], calls[m] = t1, calls[m] + 1
    return {"out": out, "x": xs, "z": raw, "scale": scale, "random": rnd, "total": np.array(total, np.int64),
            "calls": np.array(calls, np.int64)}

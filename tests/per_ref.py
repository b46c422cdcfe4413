"""Plain numpy float64 reference of prioritized replay sampling (rl/replay/prioritized_buffer.py as
hockey_amd.td3.PrioritizedRing states it), for the hkl_per_* kernels (include/hockey_learner.h, csrc/hk_learner.hip).
Nothing here imports hockey_amd.learner_hip.

Test infrastructure only.  tests/test_per_ref.py pins these functions to PrioritizedRing on the CPU;
tests/test_gpu_per.py holds the kernels to them.
"""
from fractions import Fraction

import numpy as np

W_MIN, W_MAX = np.float32(1e-6), np.float32(1e6)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 1e-9, 1e-6], np.float32)


def sanitised(w, size):
    """p [cap] float64: max(nan_to_num(w, 0, 0, 0), 1e-6f) below ``size``, 0 from there on."""
    w = np.asarray(w, np.float32)
    p = np.maximum(np.nan_to_num(w, nan=0.0, posinf=0.0, neginf=0.0), W_MIN).astype(np.float64)
    p[int(size):] = 0.0
    return p


def sample(w, size, u):
    """searchsorted(cumsum(p64), u * T, 'right') clipped to size - 1; int64 [len(u)]."""
    cdf = np.cumsum(sanitised(w, size))
    t = np.asarray(u, np.float64) * cdf[-1]
    return np.minimum(np.searchsorted(cdf, t, side="right"), int(size) - 1).astype(np.int64)


def importance(w, idx, size, beta):
    """(1 / (p_b * size)) ** beta / max, p_b = w[idx] / sum(w[idx]) on the raw weights, in float64."""
    wb = np.asarray(w, np.float32)[np.asarray(idx)].astype(np.float64)
    iw = (1.0 / ((wb / wb.sum()) * float(size))) ** float(beta)
    return iw / iw.max()


def write_back(w, idx, td):
    """numpy's own fancy assignment: of a repeated slot the last occurrence wins.  In place; returns w."""
    w[np.asarray(idx)] = np.clip(np.asarray(td, np.float32), W_MIN, W_MAX)
    return w


class RefRing:
    """The weights' bookkeeping of prioritized_buffer.py: a FIFO of ``cap`` slots starting at init_weight; a pushed
    transition takes the maximum over the slots filled after it is stored (its own old weight included)."""

    def __init__(self, cap, init_weight=1e8):
        self.cap, self.size, self.pos = int(cap), 0, 0
        self.w = np.full(self.cap, init_weight, np.float32)

    def push(self, n):
        for _ in range(n):  # one by one, as the reference's add_transition
            self.size = min(self.size + 1, self.cap)
            self.w[self.pos] = self.w[:self.size].max()
            self.pos = (self.pos + 1) % self.cap

    def sample(self, u):
        return sample(self.w, self.size, u)

    def update(self, idx, td):
        write_back(self.w, idx, td)


# ------------------------------------------------------------------------------------------------------ inputs
def capacities(blk):
    """The ring capacities of the tests for a sampler block of ``blk`` slots."""
    return [1, blk - 1, blk, blk + 1, 3 * blk + 17]


def fills(cap, blk):
    """Fill levels of a capacity, ascending: mid-block, on a block edge (where the capacity has room) and full."""
    edge = (cap // blk) * blk if cap % blk else cap - blk
    return sorted({cap, max(1, cap - blk // 3), max(1, edge)})


def dyadic_weights(size, seed, cap=None):
    """float32 weights k 2^-10, k integer in [1, 4096), the last valid one raised so that the total is a power of
    two: every float64 partial sum (below 2^22 x 2^12 x 2^-10 with 10 fractional bits) is exact in any order, and so
    is u = cdf[j] / T.  Slots from ``size`` to ``cap`` hold 1e8 (unseen)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 4096, size).astype(np.int64)
    total = int(k[:-1].sum()) + 1
    top = 1 << max(total.bit_length(), 1)
    if top - (total - 1) >= 1 << 24:  # the raised weight must stay a float32 integer multiple
        raise ValueError("size too small for an exact float32 top-up")
    k[-1] = top - (total - 1)
    w = np.full(size if cap is None else cap, 1e8, np.float32)
    w[:size] = (k.astype(np.float64) * 2.0 ** -10).astype(np.float32)
    assert np.array_equal(w[:size].astype(np.float64) * 1024, k)
    return w


def exact_draws(w, size, seed, n_random=64, limit=None):
    """u = 0, the largest double below 1, every cdf[j] / T and its predecessor (a random subset of ``limit`` slots'
    when given), and n_random uniform values: the draws of the exact-sampling checks."""
    cdf = np.cumsum(sanitised(w, size))[:size]
    rng = np.random.default_rng(seed)
    edge = cdf / cdf[-1]
    if limit is not None and size > limit:
        edge = edge[np.sort(rng.choice(size, limit, replace=False))]
    edge = edge[edge < 1.0]
    return np.concatenate([[0.0, np.nextafter(1.0, 0.0)], edge, np.nextafter(edge, 0.0), rng.random(n_random)])


def general_weights(size, regime, seed):
    """float32 lognormal weights clamped to [1e-6, 1e6]; regime "b" puts 30 % of the slots at 1e8 (unseen data);
    the first slots hold NaN, +inf, -inf, -1, 0, 1e-9 and 1e-6."""
    rng = np.random.default_rng(seed)
    w = np.clip(rng.lognormal(0.0, 2.0, size), 1e-6, 1e6).astype(np.float32)
    if regime == "b":
        w[rng.random(size) < 0.3] = np.float32(1e8)
    n = min(len(SPECIALS), size)
    w[:n] = SPECIALS[:n]
    return w


def check_general(w, size, u, idx):
    """The general-weights rule: with F the exact CDF and eps = 2 size 2^-53 T (first-order bound on any-order
    float64 summation), every draw has F[i-1] - eps <= u T <= F[i] + eps, and i is the exact index for every draw
    farther than eps from every boundary.  Returns the number of draws inside the excluded band."""
    p = sanitised(w, size)[:size]
    F = [Fraction(0)]
    for x in p:
        F.append(F[-1] + Fraction(float(x)))
    T = F[-1]
    eps = 2 * size * Fraction(1, 2 ** 53) * T
    Ff = np.array([float(f) for f in F])
    band = 0
    for ue, i in zip(u, idx):
        t = Fraction(float(ue)) * T
        i = int(i)
        assert 0 <= i < size, i
        assert F[i] - eps <= t <= F[i + 1] + eps, (ue, i)
        j = int(np.searchsorted(Ff, float(t), side="right")) - 1  # near the exact index; settle it exactly
        j = min(max(j, 0), size - 1)
        while j > 0 and F[j] > t:
            j -= 1
        while j < size - 1 and F[j + 1] <= t:
            j += 1
        near = min(abs(t - F[j]), abs(F[j + 1] - t)) <= eps
        if near:
            band += 1
        else:
            assert i == j, (ue, i, j)
    return band

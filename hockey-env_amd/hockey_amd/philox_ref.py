"""The device draws in numpy: Philox4x32-10 and the words-to-number constructions of hkl_sample, as the numpy laws of
hockey_amd.explore, hockey_amd.collect and hockey_amd.evaluator use them.  A member's (or an evaluation cell's) rows
local = 0 .. n - 1 draw the block keyed by ``seed ^ purpose`` at counter (local, calls)."""
import numpy as np

U64 = (1 << 64) - 1
_M0, _M1, _W0, _W1, LO, S32 = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9),
                               np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF), np.uint64(32))


def philox4x32_10(key, counter):
    """Philox4x32-10: key (uint64: low word k0, high word k1) and counter [..., 4] uint32 words -> [..., 4] uint32."""
    key = np.asarray(key, dtype=np.uint64)
    c = np.asarray(counter).astype(np.uint64)
    k0, k1 = key & LO, key >> S32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO, (p0 >> S32) ^ c3 ^ k1, p0 & LO
        k0, k1 = (k0 + _W0) & LO, (k1 + _W1) & LO
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def draw_words(seed, purpose, n, calls):
    """The Philox blocks [n, 4] of a member's rows local = 0 .. n - 1 at call counter ``calls``."""
    loc = np.arange(n, dtype=np.uint64)
    calls = np.uint64(int(calls) & U64)
    ctr = np.stack([loc & LO, loc >> S32, np.full(n, calls & LO), np.full(n, calls >> S32)], -1)
    return philox4x32_10(np.uint64((int(seed) & U64) ^ purpose), ctr)


def u24(words):
    """(w >> 8) 2^-24 in float32 (exact)."""
    return (words >> 8).astype(np.float32) * np.float32(2.0 ** -24)


def uniform_pm1(words):
    """2 u - 1 with u = (w >> 8) 2^-24, in float32 (exact)."""
    return np.float32(2.0) * u24(words) - np.float32(1.0)


def u53(a, b):
    """(((a << 32) | b) >> 11) 2^-53 in float64 (exact): hkl_sample's uniform."""
    bits = ((a.astype(np.uint64) << S32) | (b.astype(np.uint64) & LO)) >> np.uint64(11)
    return bits.astype(np.float64) * 2.0 ** -53


def phase_inc(words):
    """The bots' two phase increments of each block [n, 4]: 0.2 u53 of its word pairs, float64 [n, 2]."""
    return np.stack([0.2 * u53(words[:, 0], words[:, 1]), 0.2 * u53(words[:, 2], words[:, 3])], 1)


def normals(words, dtype=np.float32):
    """The four Box-Muller normals of each block (hkl_sample's construction), evaluated in ``dtype``."""
    f = np.dtype(dtype).type
    z = np.zeros(words.shape, dtype)
    for p in range(2):
        u1 = ((words[:, 2 * p] >> 8).astype(dtype) + f(0.5)) * f(2.0 ** -24)
        u2 = (words[:, 2 * p + 1] >> 8).astype(dtype) * f(2.0 ** -24)
        rad = np.sqrt(f(-2.0) * np.log(u1))
        ang = f(np.float32(2.0 * np.pi)) * u2  # the kernel's angle constant is the float32 2 pi
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z

// hk_seed.h -- the reference's seeded reset stream, restated for one lane per arena, and the reset placement law.
//
// HockeyEnv.reset(seed=s) draws its placement from gymnasium.utils.seeding.np_random(s) ==
// numpy Generator(PCG64(SeedSequence(s))) (hockey_env.py:180-181, 345-418).  Three layers, each bit for bit numpy's
// (numpy/random/bit_generator.pyx, src/pcg64/pcg64.h, _generator.pyx), held to it by tests/test_seed_ref.py:
//   seed_sequence_state  SeedSequence(seed).generate_state(4, uint64): an integer hash of the seed's uint32 words
//   Pcg64                PCG64 XSL-RR 128/64 seeded from those four words; next_double = (next64 >> 11) * 2^-53
//   seeded_placement     placement_law on Generator.uniform(lo, hi) = lo + (hi - lo) * next_double, one next64 a draw
// placement_law is the ONE statement of hockey_amd/placement.py's law in the kernels: device_placement (hk_step.h)
// passes it the Philox uniforms, seeded_placement the PCG64 ones.
//
// Single source for gfx950 (hk_seeded_reset.hip, hk_kernels.hip through hk_step.h) and for g++ (the host build and
// tests/native/seed_probe.h).  The including file defines the compile-time scene `g_scene` first, as for hk_step.h
// (the TRAIN_DEFENSE shot reads the puck's mass).  IEEE semantics are part of the contract: no FMA contraction in
// the float64 affine maps and the float32 tail, correctly rounded division and sqrtf (the library's flags).
#pragma once
#include "hk_core.h"

namespace hk {

// ------------------------------------------------------------------------------------------------
// SeedSequence (bit_generator.pyx: pool of 4 uint32 words, no spawn key)
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kSsInitA = 0x43b0d7e5u, kSsMultA = 0x931e8875u, kSsInitB = 0x8b51f9ddu, kSsMultB = 0x58f38dedu;
constexpr uint32_t kSsMixMultL = 0xca01f9ddu, kSsMixMultR = 0x4973f715u;
constexpr int kSsXshift = 16, kSsPool = 4;

HK_DEV uint32_t ss_hashmix(uint32_t v, uint32_t &hc) {
  v ^= hc;
  hc *= kSsMultA;
  v *= hc;
  v ^= v >> kSsXshift;
  return v;
}
HK_DEV uint32_t ss_mix(uint32_t x, uint32_t y) {
  uint32_t r = kSsMixMultL * x - kSsMixMultR * y;
  r ^= r >> kSsXshift;
  return r;
}

// SeedSequence(seed).generate_state(4, np.uint64) for 0 <= seed < 2^64.  The entropy is the seed's little-endian
// uint32 words without leading zero words (one for seed < 2^32, else two); a pool word with no entropy word hashes
// 0, so {lo, hi, 0, 0} is both cases.
HK_DEV void seed_sequence_state(uint64_t seed, uint64_t out[4]) {
  const uint32_t ent[kSsPool] = {(uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0u};
  uint32_t pool[kSsPool];
  uint32_t hc = kSsInitA;
#pragma unroll
  for (int i = 0; i < kSsPool; ++i) pool[i] = ss_hashmix(ent[i], hc);
#pragma unroll
  for (int src = 0; src < kSsPool; ++src)
#pragma unroll
    for (int dst = 0; dst < kSsPool; ++dst)
      if (src != dst) pool[dst] = ss_mix(pool[dst], ss_hashmix(pool[src], hc));
  // generate_state: the pool cycled into 8 uint32 words, paired little-endian
  uint32_t hb = kSsInitB, w[2 * kSsPool];
#pragma unroll
  for (int i = 0; i < 2 * kSsPool; ++i) {
    uint32_t v = pool[i % kSsPool];
    v ^= hb;
    hb *= kSsMultB;
    v *= hb;
    v ^= v >> kSsXshift;
    w[i] = v;
  }
#pragma unroll
  for (int i = 0; i < kSsPool; ++i) out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

// ------------------------------------------------------------------------------------------------
// PCG64 (pcg64.h: 128-bit LCG, XSL-RR output), the state as two uint64
// ------------------------------------------------------------------------------------------------
HK_DEV uint64_t mul64hi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

struct Pcg64 {
  uint64_t hi, lo;        // state
  uint64_t inc_hi, inc_lo;

  // state = state * 0x2360ED051FC65DA44385DF649FCCF645 + inc  (mod 2^128)
  HK_DEV void step() {
    constexpr uint64_t kMulHi = 0x2360ED051FC65DA4ull, kMulLo = 0x4385DF649FCCF645ull;
    const uint64_t plo = lo * kMulLo;
    const uint64_t phi = mul64hi(lo, kMulLo) + hi * kMulLo + lo * kMulHi;
    lo = plo + inc_lo;
    hi = phi + inc_hi + (lo < plo ? 1ull : 0ull);
  }
  // pcg64_srandom_r(initstate = s[0] << 64 | s[1], initseq = s[2] << 64 | s[3])
  HK_DEV void seed(const uint64_t s[4]) {
    hi = lo = 0ull;
    inc_hi = (s[2] << 1) | (s[3] >> 63);
    inc_lo = (s[3] << 1) | 1ull;
    step();
    const uint64_t l = lo + s[1];
    hi = hi + s[0] + (l < lo ? 1ull : 0ull);
    lo = l;
    step();
  }
  HK_DEV uint64_t next64() {
    step();
    const uint64_t v = hi ^ lo;
    const unsigned r = (unsigned)(hi >> 58);  // state >> 122
    return (v >> r) | (v << ((64u - r) & 63u));
  }
  HK_DEV double next_double() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
};

HK_DEV Pcg64 pcg64_from_seed(uint64_t seed) {
  uint64_t s[4];
  seed_sequence_state(seed, s);
  Pcg64 g;
  g.seed(s);
  return g;
}

// ------------------------------------------------------------------------------------------------
// the reset placement law (hockey_env.py:357-411, hockey_amd/placement.py)
// ------------------------------------------------------------------------------------------------
// unif(lo, hi): the next float64 uniform on [lo, hi) of the caller's stream, in the reference's draw order.
// p6 = {p2x, p2y, puckx, pucky, puck_fx, puck_fy} (float32), max_t = the mode's max_timesteps.
template <class Unif>
HK_DEV void placement_law(Unif &&unif, int mode, int one_starts, float *p6, int &max_t) {
  const double W = 10.0, H = 8.0;
  max_t = mode == 0 ? 250 : 80;
  double p2x = 4 * W / 5, p2y = H / 2;
  if (mode != 0) {
    p2x = 4 * W / 5 + unif(-W / 3, W / 6);
    p2y = H / 2 + unif(-H / 4, H / 4);
  }
  double px, py;
  float fx = 0.0f, fy = 0.0f;
  if (mode == 0 || mode == 1) {
    if (one_starts || mode == 1) {
      px = W / 2 - unif(H / 8, H / 4);
      py = H / 2 + unif(-H / 8, H / 8);
    } else {
      px = W / 2 + unif(H / 8, H / 4);
      py = H / 2 + unif(-H / 8, H / 8);
    }
  } else {
    px = W / 2 + unif(0, W / 3);
    py = H / 2 + 0.8 * unif(-H / 2, H / 2);
    float aim = (float)(H / 2 + .6 * unif(-75.0 / 60.0, 75.0 / 60.0));
    float dx = (float)px - 0.0f, dy = (float)py - aim;
    float ln = sqrtf(dx * dx + dy * dy);
    dx = dx / ln;
    dy = dy / ln;
    const float m = g_scene.mass[B_PK];
    fx = ((-dx * 60.0f) * m) / 0.02f;
    fy = ((-dy * 60.0f) * m) / 0.02f;
  }
  p6[0] = (float)p2x; p6[1] = (float)p2y; p6[2] = (float)px; p6[3] = (float)py; p6[4] = fx; p6[5] = fy;
}

// placement(mode, one_starts, np_random(seed)[0]) of hockey_amd/placement.py == HockeyEnv.reset(seed=seed)'s draws
HK_DEV void seeded_placement(uint64_t seed, int mode, int one_starts, float *p6, int &max_t) {
  Pcg64 g = pcg64_from_seed(seed);
  auto unif = [&](double lo, double hi) { return lo + (hi - lo) * g.next_double(); };
  placement_law(unif, mode, one_starts, p6, max_t);
}

}  // namespace hk

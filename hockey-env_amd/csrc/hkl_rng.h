// hkl_rng.h -- the learner library's counter-based draws, shared by the sampler (hkl_td3.h, hkl_per.h) and the
// exploration epilogue (hkl_explore.h) and the opponent draw (hkl_collect.h): Philox4x32-10 and the Box-Muller normals of one Philox block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hkl {

struct P4 {
  uint32_t x, y, z, w;
};
__device__ __forceinline__ P4 philox(uint64_t key, P4 c) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = P4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// the counter every per-sample draw uses: (sample lo, sample hi, call lo, call hi)
__device__ __forceinline__ P4 philox_at(uint64_t key, int64_t e, uint64_t ctr) {
  return philox(key, P4{(uint32_t)e, (uint32_t)(e >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32)});
}
// u = (w >> 8) 2^-24 in [0, 1)
__device__ __forceinline__ float u24(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }

// One product / one sum, each rounded on its own and never fused with a neighbour.  The library is built with
// hipcc's default contraction (fast, honouring pragmas); __fmul_rn / __fadd_rn do not stop it here -- they inline to a
// plain fmul / fadd that still carry the contract flag, and a + b * c came out as one v_fmac_f32 -- so the two
// operations are spelled under the pragma.  A numpy float32 restatement of code written with them is exact.
__device__ __forceinline__ float fmul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float fadd_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double dmul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

// four N(0, 1) draws of one block: Box-Muller on the word pairs (x, y) and (z, w) -- u1 = ((w >> 8) + 0.5) 2^-24 in
// (0, 1), u2 = (w >> 8) 2^-24, (rad cos, rad sin) with rad = sqrt(-2 ln u1) and the angle 2 pi u2
__device__ __forceinline__ void box_muller(const P4 &r, float (&z)[4]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = ((float)(w[2 * p] >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0, 1)
    const float u2 = u24(w[2 * p + 1]);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * p] = rad * cs;
    z[2 * p + 1] = rad * sn;
  }
}

}  // namespace hkl

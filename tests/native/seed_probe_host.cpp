// seed_probe_host.cpp -- seed_probe.h's per-case functions over csrc/hk_seed.h compiled for the host CPU (g++, the
// hostcheck flags).  TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>  // host-only under g++: __device__ / __forceinline__ expand to host code

#include <cmath>
#include <cstdint>
#include <cstring>

// device intrinsics hk_core.h's float64 helpers name (as in geom_probe_host.cpp)
static inline int __double2hiint(double d) { uint64_t u; std::memcpy(&u, &d, 8); return (int)(u >> 32); }
static inline double __hiloint2double(int hi, int lo) {
  const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}

#include "hk_core.h"

constexpr hk::Scene g_scene =  // the kernels' compile-time scene (hk_scene_gen.cpp)
#include "hk_scene_data.inc"
    ;

#include "hk_seed.h"

#define SP_WITH_HK
#include "seed_probe.h"

extern "C" {
void sp_state(const uint64_t *seeds, int64_t n, uint64_t *out) {
  for (int64_t i = 0; i < n; ++i) sp::state_case(seeds[i], out + 4 * i);
}
void sp_raw(const uint64_t *seeds, int64_t n, uint64_t *out) {
  for (int64_t i = 0; i < n; ++i) sp::raw_case(seeds[i], out + SP_RAW * i);
}
void sp_double(const uint64_t *seeds, int64_t n, double *out) {
  for (int64_t i = 0; i < n; ++i) sp::double_case(seeds[i], out + SP_DOUBLES * i);
}
int sp_placement(const SpCase *c, int64_t n, SpPlacement *out) {
  for (int64_t i = 0; i < n; ++i) {
    if (c[i].mode < 0 || c[i].mode > 2) return -1;
    sp::placement_case(c[i], out[i]);
  }
  return 0;
}
}

// geom_probe_host.cpp -- geom_probe.h's per-case functions over hk_geom.h compiled for the host CPU (g++, the
// hostcheck flags).  TEST INFRASTRUCTURE ONLY.  Exports the same entry points as the oracle probe.
#include <hip/hip_runtime.h>  // host-only under g++: __device__ / __forceinline__ expand to host code

#include <cmath>
#include <cstdint>
#include <cstring>

static inline int __double2hiint(double d) { uint64_t u; std::memcpy(&u, &d, 8); return (int)(u >> 32); }
static inline double __hiloint2double(int hi, int lo) {
  const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}

#ifdef GP_GEOM_HEADER  // scratch mutation runs point this at a modified copy of hk_geom.h
#include "hk_core.h"
#include GP_GEOM_HEADER
#else
#include "hk_geom.h"
#endif

#define GP_WITH_HK
#include "geom_probe.h"

constexpr hk::Scene g_scene =  // the kernels' compile-time scene (hk_scene_gen.cpp)
#include "hk_scene_data.inc"
    ;

extern "C" {
void gp_scene(GpFixture *fx, float *body4) { gp::scene_export(g_scene, fx, body4); }
int gp_distance(const GpFixture *fx, int nfx, const GpPoseCase *c, GpDistOut *o, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (c[i].fA < 0 || c[i].fA >= nfx || c[i].fB < 0 || c[i].fB >= nfx) return -1;
    gp::distance_case(fx, c[i], o[i]);
  }
  return 0;
}
int gp_toi(const GpFixture *fx, int nfx, const GpToiCase *c, GpToiOut *o, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (c[i].fA < 0 || c[i].fA >= nfx || c[i].fB < 0 || c[i].fB >= nfx) return -1;
    gp::toi_case(fx, c[i], o[i]);
  }
  return 0;
}
int gp_manifold(const GpFixture *fx, int nfx, const GpPoseCase *c, GpManOut *o, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (c[i].fA < 0 || c[i].fA >= nfx || c[i].fB < 0 || c[i].fB >= nfx) return -1;
    gp::manifold_case(fx, c[i], o[i]);
  }
  return 0;
}
}

// geom_probe.hip -- geom_probe.h's per-case functions over hk_geom.h on gfx950: one lane per case, a bounds-checked
// grid.  TEST INFRASTRUCTURE ONLY; built by `make geom-probe` with the step library's own FLAGS.
// Each launcher takes host pointers: it uploads the fixture table, the cases and the caller's PREFILLED output buffer
// (so a word the kernel does not write comes back as the caller's sentinel), launches once, and copies the outputs back.
#include "hk_geom.h"

#define GP_WITH_HK
#include "geom_probe.h"

#include <cstddef>

constexpr hk::Scene g_scene =  // the kernels' compile-time scene (hk_scene_gen.cpp); read on the host only
#include "hk_scene_data.inc"
    ;

namespace {
constexpr int kBlock = 64;  // one wave per block: a wave's 64 lanes hold 64 consecutive cases

__global__ __launch_bounds__(kBlock) void k_distance(const GpFixture *fx, const GpPoseCase *c, GpDistOut *o, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  gp::distance_case(fx, c[i], o[i]);
}
__global__ __launch_bounds__(kBlock) void k_toi(const GpFixture *fx, const GpToiCase *c, GpToiOut *o, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  gp::toi_case(fx, c[i], o[i]);
}
__global__ __launch_bounds__(kBlock) void k_manifold(const GpFixture *fx, const GpPoseCase *c, GpManOut *o, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  gp::manifold_case(fx, c[i], o[i]);
}

template <typename C>
bool indices_ok(const GpFixture *fx, int nfx, const C *c, int64_t n) {
  if (nfx <= 0 || n < 0 || n > (int64_t)1 << 24) return false;
  for (int i = 0; i < nfx; ++i)
    if (fx[i].count < 1 || fx[i].count > GP_MAXV) return false;
  for (int64_t i = 0; i < n; ++i)
    if (c[i].fA < 0 || c[i].fA >= nfx || c[i].fB < 0 || c[i].fB >= nfx) return false;
  return true;
}

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t upload(const void *src, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : 4);
    if (e != hipSuccess) return e;
    return bytes ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  }
};

template <typename C, typename O, typename K>
int run(K kernel, const GpFixture *fx, int nfx, const C *c, O *o, int64_t n) {
  if (!indices_ok(fx, nfx, c, n)) return -1;
  if (n == 0) return 0;
  DevBuf dfx, dc, dout;
  hipError_t e;
  if ((e = dfx.upload(fx, sizeof(GpFixture) * (size_t)nfx)) != hipSuccess) return (int)e;
  if ((e = dc.upload(c, sizeof(C) * (size_t)n)) != hipSuccess) return (int)e;
  if ((e = dout.upload(o, sizeof(O) * (size_t)n)) != hipSuccess) return (int)e;
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  kernel<<<blocks, kBlock>>>((const GpFixture *)dfx.p, (const C *)dc.p, (O *)dout.p, n);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(o, dout.p, sizeof(O) * (size_t)n, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
  return 0;
}
}  // namespace

extern "C" {
void gp_scene(GpFixture *fx, float *body4) { gp::scene_export(g_scene, fx, body4); }
// each returns 0, -1 for a fixture index or count out of range (nothing is launched), or the hipError_t
int gp_distance(const GpFixture *fx, int nfx, const GpPoseCase *c, GpDistOut *o, int64_t n) {
  return run(k_distance, fx, nfx, c, o, n);
}
int gp_toi(const GpFixture *fx, int nfx, const GpToiCase *c, GpToiOut *o, int64_t n) {
  return run(k_toi, fx, nfx, c, o, n);
}
int gp_manifold(const GpFixture *fx, int nfx, const GpPoseCase *c, GpManOut *o, int64_t n) {
  return run(k_manifold, fx, nfx, c, o, n);
}
}

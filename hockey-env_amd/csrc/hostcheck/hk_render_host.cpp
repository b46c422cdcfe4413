// hk_render_host.cpp -- hk_render.h (the renderer's per-pixel source) compiled for the host CPU, as a TEST HARNESS
// ONLY (tests/render_host.py, tests/native/render_sanity.cpp).  Same contract as hkr_render (include/hockey_render.h)
// on host memory: the background of shapes 1-11 is built per call with static_quad, then every frame runs
// setup_frame / dynamic_quad / quad_rgb quad by quad, exactly the kernel's path.  g++ with -ffp-contract=off on
// x86-64 SSE gives the same IEEE float results as gfx950, so the GPU test asks for byte equality.
#include <hip/hip_runtime.h>  // host-only under g++: __device__ / __forceinline__ expand to host code

#include <cstdint>
#include <cstring>
#include <vector>

static inline int __double2hiint(double d) { uint64_t u; std::memcpy(&u, &d, 8); return (int)(u >> 32); }
static inline double __hiloint2double(int hi, int lo) {
  const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}

#include "../../../include/hockey_render.h"
#include "../hk_render.h"

using namespace hkr;

extern "C" {

void hkrh_palette(uint8_t *rgb) {
  for (uint32_t k = 0; k < HKR_PALETTE_SIZE; k++) {
    const uint32_t c = palette_rgb(k);
    rgb[3 * k + 0] = (uint8_t)(c & 0xffu);
    rgb[3 * k + 1] = (uint8_t)((c >> 8) & 0xffu);
    rgb[3 * k + 2] = (uint8_t)((c >> 16) & 0xffu);
  }
}

int hkrh_render(const float *state, int64_t n_states, const int32_t *idx, int64_t m, int32_t height, int32_t width,
                int32_t format, int32_t flags, uint8_t *out, int64_t *bad_index_count) {
  if (!state || !out) return HKR_E_INVALID;
  if (height < HKR_MIN_SIZE || height > HKR_MAX_SIZE || width < HKR_MIN_SIZE || width > HKR_MAX_SIZE)
    return HKR_E_INVALID;
  if (width % kQuadPixels != 0 || (format != HKR_RGB && format != HKR_INDEX) || (flags & ~HKR_STATIC_ONLY))
    return HKR_E_INVALID;
  if (n_states < 0 || m < 0 || (!idx && m > n_states)) return HKR_E_INVALID;
  const float su = kNativeW / (float)width, sv = kNativeH / (float)height;
  const int wq = width / kQuadPixels, nq = height * wq;
  std::vector<uint32_t> bg4((size_t)nq);
  for (int q = 0; q < nq; q++) bg4[(size_t)q] = static_quad(q / wq, (q % wq) * kQuadPixels, su, sv);
  const size_t quad_bytes = format == HKR_INDEX ? 4 : 12;
  for (int64_t f = 0; f < m; f++) {
    const int64_t row = idx ? (int64_t)idx[f] : f;
    if (row < 0 || row >= n_states) {
      if (bad_index_count) *bad_index_count += 1;
      continue;
    }
    Frame F;
    if (!(flags & HKR_STATIC_ONLY)) setup_frame(state + row * 18, F);
    uint8_t *dst = out + (size_t)f * (size_t)nq * quad_bytes;
    for (int q = 0; q < nq; q++) {
      uint32_t k4 = bg4[(size_t)q];
      if (!(flags & HKR_STATIC_ONLY)) k4 = dynamic_quad(F, k4, q / wq, (q % wq) * kQuadPixels, su, sv);
      if (format == HKR_INDEX) {
        std::memcpy(dst + (size_t)q * 4, &k4, 4);
      } else {
        uint32_t d[3];
        quad_rgb(k4, d[0], d[1], d[2]);
        std::memcpy(dst + (size_t)q * 12, d, 12);
      }
    }
  }
  return HKR_OK;
}

}  // extern "C"

// hk_render.hip -- libhockey_render.so: arenas drawn on gfx950 (include/hockey_render.h; the law is hk_render.h).
//
// The kernel is store-bound (m * H * W * 3 bytes out against 72 bytes in per frame), and shaped for that:
//   * one workgroup per (frame, tile of 2048 quads = 8192 pixels: 256 lanes x 8 rounds); a lane owns 4 horizontally
//     consecutive pixels per round and writes them as whole dwords (3 for RGB, 1 for INDEX), so a wave stores
//     768 / 256 contiguous bytes per round;
//   * the frame's dynamic geometry (two racket polygons with their edge data, the puck, the three dilated bounding
//     boxes) is computed once per workgroup into LDS: one lane per racket edge on one code path in wave 0, the
//     boxes and the puck in two other waves.  A tile of 256 quads made this prologue the whole cost (a workgroup
//     waited for one lane's chain of divisions to store 3 KB); 8 rounds per workgroup amortise it
//     (scripts/render_bench.py, DESIGN.md section 3: 1.5-2 x faster at every size measured);
//   * the static layer (shapes 1-11) is not re-tested per frame: a palette-index background per (device, H, W) is
//     built once with the same per-pixel function and stays L2-resident (288 KB at native size); a lane reads its
//     background dword and runs the dynamic tests only if its span meets a bounding box.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <mutex>

#include "../../include/hockey_render.h"
#include "hk_render.h"

using namespace hkr;

namespace {

struct alignas(4) Rgb4 { uint32_t d0, d1, d2; };  // 4 pixels, 12 bytes: one global_store_dwordx3

__global__ __launch_bounds__(kTileLanes) void hkr_background_kernel(uint32_t *bg4, int nq, int wq, float su, float sv) {
  const int q = (int)blockIdx.x * kTileLanes + (int)threadIdx.x;
  if (q >= nq) return;
  const int i = q / wq, j0 = (q - i * wq) * kQuadPixels;
  bg4[q] = static_quad(i, j0, su, sv);
}

template <int FORMAT>
__global__ __launch_bounds__(kTileLanes) void hkr_render_kernel(const float *__restrict__ state, long long n_states,
                                                                const int32_t *__restrict__ idx, long long frame0,
                                                                int tiles, int nq, int wq, float su, float sv,
                                                                const uint32_t *__restrict__ bg4, int static_only,
                                                                uint8_t *__restrict__ out,
                                                                unsigned long long *bad_index_count) {
  __shared__ Frame F;
  const int tid = (int)threadIdx.x;
  const unsigned fl = blockIdx.x / (unsigned)tiles;
  const int tile = (int)(blockIdx.x - fl * (unsigned)tiles);
  const long long frame = frame0 + (long long)fl;
  const long long row = idx ? (long long)idx[frame] : frame;  // uniform over the workgroup
  if (row < 0 || row >= n_states) {
    if (tile == 0 && tid == 0 && bad_index_count) atomicAdd(bad_index_count, 1ull);
    return;
  }
  // the first background dword is requested before the geometry is set up, and each later one a round ahead
  const int q0 = tile * (kTileLanes * kTileRepeat) + tid;
  uint32_t next = q0 < nq ? bg4[q0] : 0u;
  if (!static_only) {
    const float *s = state + row * 18;
    // lanes 0..13 of wave 0: one racket edge each, on one code path; the boxes and the puck in other waves
    if (tid < 2 * kRacketVerts) {
      const int b = tid >= kRacketVerts ? 1 : 0;
      setup_racket_edge(s + 6 * b, b, tid - b * kRacketVerts, F.r[b]);
    }
    if (tid == 64 || tid == 65) setup_racket_box(s + 6 * (tid - 64), tid - 64, F.r[tid - 64]);
    if (tid == 128) setup_puck(s + 12, F.pk);
    __syncthreads();
  }
#pragma unroll 1
  for (int t = 0; t < kTileRepeat; t++) {
    // Not for ordering (F is read-only by now): a barrier keeps F's ~110 words in LDS.  Without it the compiler
    // hoists every load of the loop-invariant geometry out of this loop into registers in every lane (256 VGPRs, one
    // wave per SIMD), which measured 2.5 x slower than reading the few words a lane needs each round.
    __syncthreads();
    const int q = q0 + t * kTileLanes;
    uint32_t k4 = next;
    next = (t + 1 < kTileRepeat && q + kTileLanes < nq) ? bg4[q + kTileLanes] : 0u;
    if (q < nq) {
      if (!static_only) {
        const int i = q / wq, j0 = (q - i * wq) * kQuadPixels;
        k4 = dynamic_quad(F, k4, i, j0, su, sv);
      }
      if (FORMAT == HKR_INDEX) {
        reinterpret_cast<uint32_t *>(out)[frame * (long long)nq + q] = k4;
      } else {
        Rgb4 px;
        quad_rgb(k4, px.d0, px.d1, px.d2);
        reinterpret_cast<Rgb4 *>(out)[frame * (long long)nq + q] = px;
      }
    }
  }
}

thread_local char g_err[256];

int invalid(const char *msg) {
  snprintf(g_err, sizeof g_err, "hkr_render: %s", msg);
  return HKR_E_INVALID;
}
int device_error(hipError_t e, const char *what) {
  snprintf(g_err, sizeof g_err, "hkr_render: %s: %s", what, hipGetErrorString(e));
  return HKR_E_DEVICE;
}

// the per-size backgrounds
struct Background {
  int device, height, width;
  uint32_t *bg4;
  unsigned long long used;
};
std::mutex g_mu;
Background g_bg[HKR_CACHED_SIZES];
int g_n_bg = 0;
unsigned long long g_clock = 0;

// the background of (current device, height, width), built on first use; *out_bg4 = NULL on failure
int background(int height, int width, float su, float sv, hipStream_t stream, const uint32_t **out_bg4) {
  *out_bg4 = nullptr;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return device_error(e, "hipGetDevice");
  std::lock_guard<std::mutex> lock(g_mu);
  for (int k = 0; k < g_n_bg; k++)
    if (g_bg[k].device == dev && g_bg[k].height == height && g_bg[k].width == width) {
      g_bg[k].used = ++g_clock;
      *out_bg4 = g_bg[k].bg4;
      return HKR_OK;
    }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  e = hipStreamIsCapturing(stream, &cap);
  if (e != hipSuccess) return device_error(e, "hipStreamIsCapturing");
  if (cap != hipStreamCaptureStatusNone)
    return invalid("the first call at a size builds its background and cannot be stream-captured: render once before");
  int slot = g_n_bg;
  if (g_n_bg == HKR_CACHED_SIZES) {  // drop the least recently used size
    slot = 0;
    for (int k = 1; k < g_n_bg; k++)
      if (g_bg[k].used < g_bg[slot].used) slot = k;
    if (g_bg[slot].device != dev) (void)hipSetDevice(g_bg[slot].device);
    (void)hipDeviceSynchronize();
    (void)hipFree(g_bg[slot].bg4);
    if (g_bg[slot].device != dev) (void)hipSetDevice(dev);
    g_bg[slot] = g_bg[g_n_bg - 1];
    g_n_bg--;
    slot = g_n_bg;
  }
  const int nq = height * width / kQuadPixels;
  uint32_t *bg4 = nullptr;
  e = hipMalloc((void **)&bg4, (size_t)nq * sizeof(uint32_t));
  if (e != hipSuccess) return device_error(e, "hipMalloc of the background");
  hipLaunchKernelGGL(hkr_background_kernel, dim3((unsigned)((nq + kTileLanes - 1) / kTileLanes)), dim3(kTileLanes), 0,
                     stream, bg4, nq, width / kQuadPixels, su, sv);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(stream);  // other streams may read it from now on
  if (e != hipSuccess) {
    (void)hipFree(bg4);
    return device_error(e, "building the background");
  }
  g_bg[slot] = Background{dev, height, width, bg4, ++g_clock};
  g_n_bg++;
  *out_bg4 = bg4;
  return HKR_OK;
}

}  // namespace

extern "C" {

const char *hkr_last_error(void) { return g_err; }

void hkr_palette(uint8_t *rgb) {
  if (!rgb) return;
  for (uint32_t k = 0; k < HKR_PALETTE_SIZE; k++) {
    const uint32_t c = palette_rgb(k);
    rgb[3 * k + 0] = (uint8_t)(c & 0xffu);
    rgb[3 * k + 1] = (uint8_t)((c >> 8) & 0xffu);
    rgb[3 * k + 2] = (uint8_t)((c >> 16) & 0xffu);
  }
}

int hkr_render(const float *state, int64_t n_states, const int32_t *idx, int64_t m, int32_t height, int32_t width,
               int32_t format, int32_t flags, uint8_t *out, int64_t *bad_index_count, void *stream) {
  if (!state) return invalid("state is NULL");
  if (!out) return invalid("out is NULL");
  if (((uintptr_t)out & 3u) != 0) return invalid("out is not 4-byte aligned");
  if (height < HKR_MIN_SIZE || height > HKR_MAX_SIZE || width < HKR_MIN_SIZE || width > HKR_MAX_SIZE)
    return invalid("height and width must lie in [4, 4096]");
  if (width % kQuadPixels != 0) return invalid("width must be a multiple of 4");
  if (format != HKR_RGB && format != HKR_INDEX) return invalid("unknown format");
  if (flags & ~HKR_STATIC_ONLY) return invalid("unknown flags");
  if (n_states < 0 || m < 0) return invalid("negative count");
  if (!idx && m > n_states) return invalid("idx is NULL and m exceeds n_states");
  if (m == 0) return HKR_OK;
  const float su = kNativeW / (float)width, sv = kNativeH / (float)height;
  const uint32_t *bg4 = nullptr;
  const int rc = background(height, width, su, sv, (hipStream_t)stream, &bg4);
  if (rc != HKR_OK) return rc;
  const int nq = height * width / kQuadPixels, wq = width / kQuadPixels;
  const int tile_quads = kTileLanes * kTileRepeat, tiles = (nq + tile_quads - 1) / tile_quads;
  // a launch holds at most 2^22 workgroups (2^30 lanes): more frames go out in consecutive launches
  const int64_t per_launch = (int64_t)(1 << 22) / tiles > 0 ? (int64_t)(1 << 22) / tiles : 1;
  for (int64_t f0 = 0; f0 < m; f0 += per_launch) {
    const int64_t nf = m - f0 < per_launch ? m - f0 : per_launch;
    const dim3 grid((unsigned)(nf * tiles)), block(kTileLanes);
    if (format == HKR_INDEX)
      hipLaunchKernelGGL(hkr_render_kernel<HKR_INDEX>, grid, block, 0, (hipStream_t)stream, state, (long long)n_states,
                         idx, (long long)f0, tiles, nq, wq, su, sv, bg4, flags & HKR_STATIC_ONLY, out,
                         (unsigned long long *)bad_index_count);
    else
      hipLaunchKernelGGL(hkr_render_kernel<HKR_RGB>, grid, block, 0, (hipStream_t)stream, state, (long long)n_states,
                         idx, (long long)f0, tiles, nq, wq, su, sv, bg4, flags & HKR_STATIC_ONLY, out,
                         (unsigned long long *)bad_index_count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return device_error(e, "launch");
  }
  return HKR_OK;
}

void hkr_release(void) {
  std::lock_guard<std::mutex> lock(g_mu);
  int dev = 0;
  const bool have_dev = hipGetDevice(&dev) == hipSuccess;
  for (int k = 0; k < g_n_bg; k++) {
    if (hipSetDevice(g_bg[k].device) != hipSuccess) continue;
    (void)hipDeviceSynchronize();
    (void)hipFree(g_bg[k].bg4);
  }
  g_n_bg = 0;
  if (have_dev) (void)hipSetDevice(dev);
}

}  // extern "C"

// render_sanity.cpp -- the renderer's host build (csrc/hostcheck/hk_render_host.cpp, i.e. csrc/hk_render.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/test_render_law.py compiles and
// runs it).  Every frame is rendered into a heap buffer of exactly its size, so a store past a frame's end, a read
// past the state rows or a wild idx row is a sanitizer report.
//
//   render_sanity STATES.bin     STATES.bin = n rows of 18 float32 (hk_get_state layout)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hockey_render.h"

extern "C" int hkrh_render(const float *state, int64_t n_states, const int32_t *idx, int64_t m, int32_t height,
                           int32_t width, int32_t format, int32_t flags, uint8_t *out, int64_t *bad_index_count);
extern "C" void hkrh_palette(uint8_t *rgb);

static int fail(const char *what, int h, int w) {
  std::printf("render sanity: FAILED %s at %d x %d\n", what, h, w);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage", 0, 0);
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return fail("open", 0, 0);
  std::vector<float> state;
  float row[18];
  while (std::fread(row, sizeof(float), 18, f) == 18) state.insert(state.end(), row, row + 18);
  std::fclose(f);
  const int64_t n = (int64_t)(state.size() / 18);
  if (n < 4) return fail("too few states", 0, 0);
  uint8_t pal[HKR_PALETTE_SIZE * 3];
  hkrh_palette(pal);

  const int sizes[3][2] = {{480, 600}, {120, 152}, {84, 84}};
  for (const auto &hw : sizes) {
    const int h = hw[0], w = hw[1];
    const size_t px = (size_t)h * (size_t)w;
    for (int flags = 0; flags <= HKR_STATIC_ONLY; flags++) {
      std::vector<uint8_t> index((size_t)n * px), rgb((size_t)n * px * 3);
      int64_t bad = 0;
      if (hkrh_render(state.data(), n, nullptr, n, h, w, HKR_INDEX, flags, index.data(), &bad) != HKR_OK || bad)
        return fail("index render", h, w);
      if (hkrh_render(state.data(), n, nullptr, n, h, w, HKR_RGB, flags, rgb.data(), &bad) != HKR_OK || bad)
        return fail("rgb render", h, w);
      for (size_t k = 0; k < (size_t)n * px; k++) {
        if (index[k] >= HKR_PALETTE_SIZE) return fail("palette index range", h, w);
        if (std::memcmp(&rgb[3 * k], &pal[3 * index[k]], 3) != 0) return fail("palette[index] == rgb", h, w);
      }
    }
    // a bad index leaves its frame untouched and counts once; good ones around it are drawn
    const int32_t idx[5] = {(int32_t)(n - 1), (int32_t)n, 0, -1, (int32_t)(n - 1)};
    std::vector<uint8_t> out(5 * px * 3, 0xA5), one(px * 3);
    int64_t bad = 0;
    if (hkrh_render(state.data(), n, idx, 5, h, w, HKR_RGB, 0, out.data(), &bad) != HKR_OK) return fail("idx render", h, w);
    if (bad != 2) return fail("bad index count", h, w);
    for (int k = 0; k < 5; k++) {
      const uint8_t *frame = out.data() + (size_t)k * px * 3;
      if (idx[k] < 0 || idx[k] >= n) {
        for (size_t b = 0; b < px * 3; b++)
          if (frame[b] != 0xA5) return fail("bad index frame touched", h, w);
      } else {
        int64_t none = 0;
        if (hkrh_render(state.data() + (size_t)idx[k] * 18, 1, nullptr, 1, h, w, HKR_RGB, 0, one.data(), &none) != HKR_OK)
          return fail("single render", h, w);
        if (std::memcmp(frame, one.data(), px * 3) != 0) return fail("idx frame differs from its row's", h, w);
      }
    }
  }
  // rejected arguments reach no pixel
  uint8_t tiny[16];
  if (hkrh_render(state.data(), n, nullptr, 1, 4, 6, HKR_RGB, 0, tiny, nullptr) != HKR_E_INVALID) return fail("width % 4", 4, 6);
  if (hkrh_render(state.data(), n, nullptr, 1, 2, 4, HKR_RGB, 0, tiny, nullptr) != HKR_E_INVALID) return fail("height < 4", 2, 4);
  if (hkrh_render(state.data(), n, nullptr, n + 1, 4, 4, HKR_INDEX, 0, tiny, nullptr) != HKR_E_INVALID) return fail("m > n", 4, 4);
  if (hkrh_render(nullptr, n, nullptr, 1, 4, 4, HKR_INDEX, 0, tiny, nullptr) != HKR_E_INVALID) return fail("null state", 4, 4);
  std::printf("render sanity: ok (%lld states)\n", (long long)n);
  return 0;
}

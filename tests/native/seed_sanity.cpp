// seed_sanity.cpp -- csrc/hk_seed.h under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program
// (tests/test_seed_ref.py compiles and runs it; it is never loaded into python).  Every case of the list runs
// through all three layers -- the 128-bit LCG carried as two uint64, the rotation by state >> 122 (0 included) and
// the uint32 hash are where undefined behaviour could hide -- and each placement is compared with the expected one.
//
//   seed_sanity CASES.bin WANT.bin     CASES.bin = n SpCase rows, WANT.bin = n SpPlacement rows (seed_probe.h)
#include <hip/hip_runtime.h>  // host-only under g++

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// device intrinsics hk_core.h's float64 helpers name (as in geom_probe_host.cpp)
static inline int __double2hiint(double d) { uint64_t u; std::memcpy(&u, &d, 8); return (int)(u >> 32); }
static inline double __hiloint2double(int hi, int lo) {
  const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}

#include "hk_core.h"

constexpr hk::Scene g_scene =
#include "hk_scene_data.inc"
    ;

#include "hk_seed.h"

#define SP_WITH_HK
#include "seed_probe.h"

template <class T>
static bool read_rows(const char *path, std::vector<T> &rows) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  T r;
  while (std::fread(&r, sizeof(T), 1, f) == 1) rows.push_back(r);
  std::fclose(f);
  return true;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("seed sanity: FAILED usage\n");
    return 1;
  }
  std::vector<SpCase> cases;
  std::vector<SpPlacement> want;
  if (!read_rows(argv[1], cases) || !read_rows(argv[2], want) || cases.empty() || cases.size() != want.size()) {
    std::printf("seed sanity: FAILED reading the case files\n");
    return 1;
  }
  uint64_t fold = 0;
  for (size_t i = 0; i < cases.size(); ++i) {
    // exact-size heap rows: a store past any of them is an AddressSanitizer report
    std::vector<uint64_t> st(4), raw(SP_RAW);
    std::vector<double> dbl(SP_DOUBLES);
    sp::state_case(cases[i].seed, st.data());
    sp::raw_case(cases[i].seed, raw.data());
    sp::double_case(cases[i].seed, dbl.data());
    for (int k = 0; k < SP_DOUBLES; ++k)
      if (!(dbl[k] >= 0.0 && dbl[k] < 1.0)) {
        std::printf("seed sanity: FAILED next_double outside [0, 1) at case %zu\n", i);
        return 1;
      }
    fold ^= st[0] ^ raw[SP_RAW - 1];
    SpPlacement got;
    std::memset(&got, 0, sizeof(got));
    sp::placement_case(cases[i], got);
    if (std::memcmp(got.p6, want[i].p6, sizeof(got.p6)) != 0 || got.max_t != want[i].max_t) {
      std::printf("seed sanity: FAILED placement differs at case %zu (seed %llu mode %d one %d)\n", i,
                  (unsigned long long)cases[i].seed, cases[i].mode, cases[i].one_starts);
      return 1;
    }
  }
  std::printf("seed sanity: ok (%zu cases, fold %016llx)\n", cases.size(), (unsigned long long)fold);
  return 0;
}

/* seed_probe.h -- one record layout and one per-case function for each layer of csrc/hk_seed.h (SeedSequence state,
 * PCG64 raw words and doubles, the seeded reset placement).  TEST INFRASTRUCTURE ONLY: the product never loads it.
 *
 * Two host builds use it (tests/seed_cases.py holds the numpy dtypes):
 *   seed_probe_host.cpp   a shared library under g++ with the host flags, loaded by tests/test_seed_ref.py
 *   seed_sanity.cpp       a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
 * The gfx950 build of the same header is the product's own kernel (csrc/hk_seeded_reset.hip), tested through
 * hk_seeded_params / hk_reset_seeded. */
#ifndef SEED_PROBE_H
#define SEED_PROBE_H
#include <stdint.h>

#define SP_RAW 8     /* next64 words recorded per seed */
#define SP_DOUBLES 5 /* next_double values recorded per seed (a reset draws at most five) */

typedef struct { uint64_t seed; int32_t mode, one_starts; } SpCase;     /* 16 bytes */
typedef struct { float p6[6]; int32_t max_t; int32_t pad; } SpPlacement; /* 32 bytes */

#if defined(__cplusplus) && defined(SP_WITH_HK)
/* the including file has included hk_core.h, defined g_scene and included hk_seed.h */
namespace sp {
inline void state_case(uint64_t seed, uint64_t *out4) { hk::seed_sequence_state(seed, out4); }
inline void raw_case(uint64_t seed, uint64_t *out) {
  hk::Pcg64 g = hk::pcg64_from_seed(seed);
  for (int k = 0; k < SP_RAW; ++k) out[k] = g.next64();
}
inline void double_case(uint64_t seed, double *out) {
  hk::Pcg64 g = hk::pcg64_from_seed(seed);
  for (int k = 0; k < SP_DOUBLES; ++k) out[k] = g.next_double();
}
inline void placement_case(const SpCase &c, SpPlacement &o) {
  int mt = 0;
  hk::seeded_placement(c.seed, c.mode, c.one_starts, o.p6, mt);
  o.max_t = mt;
  o.pad = 0;
}
}  // namespace sp
#endif

#endif

// hk_hostcheck.cpp -- the per-arena device code (hk_step.h / hk_arena.h / hk_solver.h / hk_velocity.h / hk_geom.h)
// compiled for the host CPU, as a DEBUG AND TEST HARNESS ONLY.
//
// It lets the CPU test suite run the kernel's own per-lane logic against the oracle without a GPU, and
// gives gdb a build of the physics (GPU debuggers are unavailable on the pool).  It is never loaded by
// the product package (hockey_amd refuses to run without libhockey_hip.so and has no CPU path); only
// tests/ and scripts/ use libhockey_hostcheck.so.  The code is the same source as the kernel: g++ with
// -ffp-contract=off on x86-64 SSE gives the same IEEE float/double results as gfx950 (correctly rounded
// +,-,*,/,sqrt; no contraction), which the parity tests check.
#include <hip/hip_runtime.h>  // host-only under g++: __device__ / __forceinline__ expand to host code

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

static inline int __float_as_int(float x) { int r; std::memcpy(&r, &x, 4); return r; }
static inline unsigned __float_as_uint(float x) { unsigned r; std::memcpy(&r, &x, 4); return r; }
static inline float __int_as_float(int x) { float r; std::memcpy(&r, &x, 4); return r; }
static inline float __uint_as_float(unsigned x) { float r; std::memcpy(&r, &x, 4); return r; }
static inline int __ffs(unsigned x) { return __builtin_ffs((int)x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
static inline int __double2hiint(double d) { uint64_t u; std::memcpy(&u, &d, 8); return (int)(u >> 32); }
static inline double __hiloint2double(int hi, int lo) {
  const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}

#define HK_HOST_DIAG
#include "../hk_core.h"

constexpr hk::Scene g_scene =  // the kernels' compile-time scene (hk_scene_gen.cpp)
#include "../hk_scene_data.inc"
    ;

#define SLDS g_scene  // the host build reads the one scene copy
#include "../hk_step.h"
#include "../hk_arena_copy.h"

unsigned long long hk::g_hk_host_diag[4];
unsigned long long hk::g_hk_host_toi_lean;
unsigned long long hk::g_hk_flop_ev[hk::EV_N];

using namespace hk;

struct HostCtx {
  int64_t n;
  std::vector<float> f, man, ws;
  std::vector<int32_t> i;
  std::vector<double> phase;
  std::vector<unsigned long long> counters;
  std::vector<float> lds;
  DevState s;
  KCfg cfg;
};

extern "C" {

// cfg = {keep_mode, mode, auto_reset, vel_ref, policy0, policy1, diag_flags}; seed; arena_offset
void *hkh_create(int64_t n, const int *cfg6, uint64_t seed, int64_t arena_offset) {
  HostCtx *c = new HostCtx();
  c->n = n;
  c->f.assign((size_t)NFF * n, 0.0f);
  c->i.assign((size_t)NPW * n, 0);
  c->man.assign((size_t)NSOLID * NMF * n, 0.0f);
  c->phase.assign((size_t)3 * n, 0.0);
  c->counters.assign(16, 0ull);
  c->lds.assign((size_t)kLdsWords, 0.0f);
  c->s.f = c->f.data();
  c->s.i = c->i.data();
  c->s.man = c->man.data();
  c->ws.assign((size_t)kBigC * kSlotWords * n, 0.0f);
  c->s.ws = c->ws.data();
  c->s.phase = c->phase.data();
  c->s.counters = c->counters.data();
  c->s.n = n;
  std::memset(&c->cfg, 0, sizeof(c->cfg));
  c->cfg.keep_mode = cfg6[0];
  c->cfg.mode = cfg6[1];
  c->cfg.auto_reset = cfg6[2];
  c->cfg.vel_ref = cfg6[3];
  c->cfg.policy[0] = cfg6[4];
  c->cfg.policy[1] = cfg6[5];
  c->cfg.seed = seed;
  c->cfg.arena_offset = arena_offset;
  c->cfg.diag = cfg6[6];
  for (int64_t a = 0; a < n; ++a) init_lane(c->s, c->cfg, a);
  return c;
}

void hkh_destroy(void *h) { delete (HostCtx *)h; }

void hkh_reset(void *h, const uint8_t *mask, const float *params, const int32_t *max_t, const uint8_t *one) {
  HostCtx *c = (HostCtx *)h;
  for (int64_t a = 0; a < c->n; ++a)
    if (!mask || mask[a]) reset_lane(c->s, c->cfg, a, params, max_t, one);
}

// io layout == StepIO (same field order as include/hockey.h's hk_step_io)
void hkh_step(void *h, const StepIO *io) {
  HostCtx *c = (HostCtx *)h;
  for (int64_t a = 0; a < c->n; ++a) {
    PhaseT T;
    LaneOut out;
    StepWords m;
    fetch_words(m, c->s, c->cfg, *io, a);
    step_lane(c->s, c->cfg, *io, a, c->lds.data(), (int)(a & 63), T, out, m);
    c->counters[0] += 1;
    c->counters[1] += out.done_edge;
    c->counters[2] += out.win1;
    c->counters[3] += out.win2;
    c->counters[4] += out.ntoi;
    c->counters[5] += out.ovf;
    c->counters[6] += out.nbig;
    c->counters[7] += out.bad_policy;
    c->counters[9] += out.bad_action;
  }
}

void hkh_get_state(void *h, float *st, int32_t *aux) {
  HostCtx *c = (HostCtx *)h;
  for (int64_t a = 0; a < c->n; ++a) get_state_lane(c->s, a, st, aux);
}

void hkh_set_state(void *h, const uint8_t *mask, const float *st, const int32_t *aux) {
  HostCtx *c = (HostCtx *)h;
  for (int64_t a = 0; a < c->n; ++a)
    if (!mask || mask[a]) set_state_lane(c->s, c->cfg, a, st, aux);
}

void hkh_observe(void *h, float *obs, float *obs2) {
  HostCtx *c = (HostCtx *)h;
  for (int64_t a = 0; a < c->n; ++a) observe_lane(c->s, c->cfg, a, obs, obs2);
}

// BasicOpponent phases [N][3] (DevState::phase is [3][N]): player 1, player 2, player 2's weak bot under an override
void hkh_phase(void *h, double *out) {
  HostCtx *c = (HostCtx *)h;
  for (int64_t a = 0; a < c->n; ++a)
    for (int r = 0; r < 3; ++r) out[a * 3 + r] = c->phase[(size_t)r * c->n + a];
}

// raw SoA state (diagnostics): f [NFF][N] floats, i [NPW][N] packed int words
void hkh_raw(void *h, float **f, int32_t **i) {
  HostCtx *c = (HostCtx *)h;
  *f = c->f.data();
  *i = c->i.data();
}

// event counts of the algorithmic FLOP count (hk_core.h HK_EV), process-wide; read and cleared
void hkh_flop_events(unsigned long long *out) {
  std::memcpy(out, hk::g_hk_flop_ev, sizeof(hk::g_hk_flop_ev));
  std::memset(hk::g_hk_flop_ev, 0, sizeof(hk::g_hk_flop_ev));
}
int hkh_flop_event_count(void) { return hk::EV_N; }

// velocity-loop coverage counters (hk_solver.h HK_HOST_DIAG_INC, counted in hk_velocity.h), process-wide; read and cleared
void hkh_diag(unsigned long long *out4) {
  std::memcpy(out4, hk::g_hk_host_diag, sizeof(hk::g_hk_host_diag));
  std::memset(hk::g_hk_host_diag, 0, sizeof(hk::g_hk_host_diag));
}

// TOI events that took the lean one-contact path (hk_world.h toi_island_solve_one), process-wide; read and cleared
unsigned long long hkh_toi_lean(void) {
  const unsigned long long n = hk::g_hk_host_toi_lean;
  hk::g_hk_host_toi_lean = 0ull;
  return n;
}

// ---- exact arena copies (hk_arena_copy.h): the kernel's copy_entry / copy_arena, one list entry after the other ----
constexpr int kCntBadIndex = 8;  // HK_CNT_BAD_INDEX (include/hockey.h)
static void copy_list(const ArenaView &dst, const int64_t *dst_idx, const ArenaView &src, const int64_t *src_idx,
                      int64_t m, unsigned long long *bad) {
  for (int64_t e = 0; e < m; ++e) {
    int64_t di, si;
    if (copy_entry(dst, dst_idx, src, src_idx, e, di, si))
      copy_arena(dst, di, src, si);
    else
      *bad += 1;
  }
}

int64_t hkh_snapshot_bytes(int64_t m) { return m < 0 ? 0 : blob_layout(m).bytes; }

void hkh_snapshot_layout(int32_t *out5) {
  out5[0] = NFF;
  out5[1] = NPW;
  out5[2] = kPhaseRows;
  out5[3] = NSOLID;
  out5[4] = NMF;
}

// 0, or -1 for a blob that is not 16-byte aligned (as hk_snapshot / hk_restore: HK_E_INVALID)
int hkh_snapshot(void *h, const int64_t *idx, int64_t m, void *blob) {
  HostCtx *c = (HostCtx *)h;
  if (m < 0 || ((uintptr_t)blob & 15)) return -1;
  copy_list(blob_view(blob, m), nullptr, view_of(c->s), idx, m, &c->counters[kCntBadIndex]);
  return 0;
}

int hkh_restore(void *h, const int64_t *idx, int64_t m, const void *blob, int64_t blob_m, const int64_t *rows) {
  HostCtx *c = (HostCtx *)h;
  if (m < 0 || blob_m < 0 || ((uintptr_t)blob & 15)) return -1;
  copy_list(view_of(c->s), idx, blob_view(const_cast<void *>(blob), blob_m), rows, m, &c->counters[kCntBadIndex]);
  return 0;
}

// -1 for contexts that differ in keep_mode or vel_ref (as hk_copy_arenas)
int hkh_copy_arenas(void *dh, const int64_t *dst_idx, void *sh, const int64_t *src_idx, int64_t m) {
  HostCtx *d = (HostCtx *)dh, *s = (HostCtx *)sh;
  if (m < 0 || d->cfg.keep_mode != s->cfg.keep_mode || d->cfg.vel_ref != s->cfg.vel_ref) return -1;
  copy_list(view_of(d->s), dst_idx, view_of(s->s), src_idx, m, &d->counters[kCntBadIndex]);
  return 0;
}

void hkh_counters(void *h, unsigned long long *out16) {
  HostCtx *c = (HostCtx *)h;
  std::memcpy(out16, c->counters.data(), 16 * sizeof(unsigned long long));
}

}  // extern "C"

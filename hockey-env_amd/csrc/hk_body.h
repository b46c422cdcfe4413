// hk_body.h -- the register body file of one arena: one arena per lane, register-resident (v3 of the step kernel).
//
// State layout per lane:
//   * the 3 dynamic bodies live in register arrays (Dyn), indexed with compile-time indices or through
//     3-way selects for a runtime body id; static bodies are compile-time scene data (constexpr Scene,
//     and its LDS copy for per-lane ids);
//   * contact state is bitmasks over the 27-pair table (touching / enabled / TOI / island flags);
//   * Box2D manifolds stay in HBM (DevState::man, 64-B records [slot][arena], see man_rec) and are read
//     or written in place where Box2D reads or writes them;
//   * per-pair TOI alphas / sub-step counts and the static bodies' sweep alpha0 live in LDS
//     ([k][64 lanes], conflict-free for any k);
//   * pair loops are uniform across the wave, so scene data arrives through scalar loads.
// Nothing in the step touches private (scratch) memory.  Float operation order is the oracle's.
#pragma once
#include "hk_geom.h"
#include "hk_kernels.h"

namespace hk {

#define SC g_scene
// The scene again, as the step kernel's LDS copy (hk_kernels.hip: g_scene_lds, filled at kernel start).
// Scene data indexed by a per-lane (divergent) pair / fixture / body id is read from here: a ds_read instead
// of a gather through the vector L1 from the code object's constant table.  Compile-time and wave-uniform
// indices keep using SC (instruction literals / scalar loads).
#ifndef SLDS
#define SLDS g_scene_lds
#endif

// register-resident solver slots.  Strong-vs-strong statistics (host build, 2.4M arena-steps): island
// solves with 0/1/2/3/4+ contacts 70.3/29.7/1.5/0.02/3e-4 %, TOI mini-islands with 1/2 contacts
// 99.7/0.3 %.  Larger solves take the HBM slot file (HbmSlots), bit-identically.
constexpr int kIslandC = 4;
constexpr int kToiC = 2;
constexpr int kBigC = kMaxIsland;  // generic solver bound (geometric max is 9)
constexpr uint32_t kEdgeMask[3] = {(1u << 8) | (1u << 10) | (0xFFu << 11),   // player1: 8, 10, 11..18
                                   (1u << 9) | (1u << 10) | (0xFFu << 19),   // player2: 9, 10, 19..26
                                   0x3FFu};                                  // puck: 0..9
constexpr uint32_t kSensorMask = (1u << 6) | (1u << 7);
// pairs that take part in continuous collision: static A, not a sensor (Box2D: a non-bullet dynamic pair
// and sensors never get a TOI)
constexpr uint32_t kToiPairs = 0x7FFFFFFu & ~kSensorMask & ~((1u << 8) | (1u << 9) | (1u << 10));
constexpr uint32_t pair_mask_of_scene(bool toi) {
  uint32_t m = 0u;
  for (int p = 0; p < NP; ++p)
    if (toi ? (!g_scene.sensor[p] && g_scene.pbodyA[p] >= 3) : g_scene.sensor[p] != 0) m |= 1u << p;
  return m;
}
static_assert(pair_mask_of_scene(true) == kToiPairs && pair_mask_of_scene(false) == kSensorMask,
              "pair masks follow the compiled scene's pair table");

// LDS per lane: [0,27) TOI alpha per pair, [27,35) static sweep alpha0, [35,62) TOI sub-step count; then,
// per wave, the work list of the cooperative b2TimeOfImpact drain (toi_drain_wave): kToiQ items of
// kToiItemWords words
constexpr int kLdsToi = 0, kLdsSal0 = 27, kLdsCnt = 35, kLdsPerLane = 62;
constexpr int kToiQ = 128, kToiItemWords = 9;
constexpr int kLdsWords = kLdsPerLane * 64 + kToiQ * kToiItemWords;

struct Dyn {
  float px[3], py[3], qs[3], qc[3];      // transform (origin, rotation)
  float cx[3], cy[3], a[3];              // sweep c, a (COM, angle)
  float c0x[3], c0y[3], a0[3], al0[3];   // sweep c0, a0, alpha0
  float vx[3], vy[3], w[3];
  float fx[3], fy[3], tq[3];
  float ld[3], ad[3], sleep[3];
  int awake[3];
};

struct Arena {
  Dyn d;
  uint32_t touch, enabled, toiflag, cisl, bisl;
  int keep_mode, max_t, time, done, winner, has1, has2, vel_ref;
  int force_big;  // diagnostics: always take the generic (large-island) solver
  int n_toi, overflow, n_big;  // TOI events, island overflow flag, large-island (generic) solves
#ifdef HK_PHASE_TIMERS
  int dg_vit_isl, dg_vit_toi, dg_pit, dg_toi_calls, dg_nc_max;  // diagnostics build: per-lane work
  int dg_toi_lean;  // TOI events of this lane that took the lean one-contact path (toi_island_solve_one)
#endif
  float *man;   // HBM manifolds
  float *ws;    // HBM slot workspace of large islands (HbmSlots)
  int64_t n, a;
  float *lds;   // this wave's LDS block
  int lane;
#ifdef HK_TRACE
  float *trace;  // diagnostic build: per-phase snapshots (HK_TRACE_POINT)
#endif
};

// Diagnostic build only (make TRACE=1): snapshot the arena after phase k into io.debug[a][13 + 24k ...].
#ifdef HK_TRACE
constexpr int kTraceStride = 13 + 24 * 4 + 128;
HK_DEV void trace_point(const Arena &w, int k) {
  if (!w.trace) return;
  float *t = w.trace + 13 + 24 * k;
  for (int b = 0; b < 3; ++b) {
    t[6 * b + 0] = w.d.px[b]; t[6 * b + 1] = w.d.py[b]; t[6 * b + 2] = w.d.a[b];
    t[6 * b + 3] = w.d.vx[b]; t[6 * b + 4] = w.d.vy[b]; t[6 * b + 5] = w.d.w[b];
  }
  t[18] = __int_as_float((int)w.touch);
  t[19] = __int_as_float((int)w.enabled);
  t[20] = __int_as_float(w.d.awake[0] | (w.d.awake[1] << 1) | (w.d.awake[2] << 2));
  t[21] = (float)w.n_toi;
  t[22] = (float)w.n_big;
  t[23] = __int_as_float((int)w.cisl);
}
#define HK_TRACE_POINT(w, k) trace_point(w, k)
#define HK_TRACE_SLOT(w, k, s)                                              \
  do {                                                                      \
    if ((w).trace) {                                                        \
      const float *_src = reinterpret_cast<const float *>(&(s));            \
      for (int _q = 0; _q < 64 && _q < (int)(sizeof(s) / 4); ++_q)          \
        (w).trace[13 + 96 + 64 * (k) + _q] = _src[_q];                      \
    }                                                                       \
  } while (0)
#else
#define HK_TRACE_SLOT(w, k, s) ((void)0)
#define HK_TRACE_POINT(w, k) ((void)0)
#endif

// ------------------------------------------------------------------------------------------------
// runtime-id access to the register body file (3-way selects, static -> default)
// ------------------------------------------------------------------------------------------------
// Operands are read into locals first so clang emits straight-line selects (v_cndmask) instead of the
// branch trees it generates for conditional operators over memory operands.
template <typename T>
HK_DEV T pick(const T (&x)[3], int b, T dflt) {
  const T x0 = x[0], x1 = x[1], x2 = x[2];
  T r = dflt;
  r = (b == 2) ? x2 : r;
  r = (b == 1) ? x1 : r;
  r = (b == 0) ? x0 : r;
  return r;
}
template <typename T>
HK_DEV void place(T (&x)[3], int b, T v) {
  const T x0 = x[0], x1 = x[1], x2 = x[2];
  x[0] = (b == 0) ? v : x0;
  x[1] = (b == 1) ? v : x1;
  x[2] = (b == 2) ? v : x2;
}
// Pair sides (build_scene): body A is player 1, player 2 or a static body, never the puck; body B is a
// dynamic body.  The side-specific selects drop the comparisons that can never hold (velocity-loop VALU).
constexpr bool pair_sides_ok() {
  for (int p = 0; p < NP; ++p)
    if (g_scene.pbodyA[p] == B_PK || g_scene.pbodyB[p] > B_PK) return false;
  return true;
}
static_assert(pair_sides_ok(), "pair body A is never the puck, pair body B is always dynamic");
template <typename T>
HK_DEV T pick_a(const T (&x)[3], int b, T dflt) {
  const T x0 = x[0], x1 = x[1];
  T r = (b == 1) ? x1 : dflt;
  r = (b == 0) ? x0 : r;
  return r;
}
template <typename T>
HK_DEV T pick_b(const T (&x)[3], int b) {
  const T x0 = x[0], x1 = x[1], x2 = x[2];
  T r = (b == 1) ? x1 : x2;
  r = (b == 0) ? x0 : r;
  return r;
}
template <typename T>
HK_DEV void place_a(T (&x)[3], int b, T v) {
  const T x0 = x[0], x1 = x[1];
  x[0] = (b == 0) ? v : x0;
  x[1] = (b == 1) ? v : x1;
}
HK_DEV float &LDS(Arena &w, int k) { return w.lds[k * 64 + w.lane]; }
// Box2D manifold record of solid-pair slot `slot` for this arena: [slot][arena][16 words].  A lane's
// record is one 64-B block, so the per-lane (divergent) slot accesses of the near-pair / island / TOI
// queues touch one cache line per record instead of one per field; lanes on the same slot read 4 KiB
// contiguous per wave.  Accesses are whole 16-B quads (global_load/store_dwordx4).
struct alignas(16) Quad { float x, y, z, w; };
HK_DEV Quad *man_rec(const Arena &w, int slot) {
  return reinterpret_cast<Quad *>(w.man + ((int64_t)slot * w.n + w.a) * NMF);
}

// per-lane body id -> dynamic-body constants by select (a static body reads 0)
HK_DEV float inv_mass(int b) { return pick(SC.invMass, b, 0.0f); }
HK_DEV float inv_inertia(int b) { return pick(SC.invI, b, 0.0f); }
HK_DEV v2 local_center(int b) { return V(pick(SC.lcx, b, 0.0f), pick(SC.lcy, b, 0.0f)); }

HK_DEV xform body_xf(const Arena &w, int b) {
  xform x;
  if (b < 3) {
    x.p = V(pick(w.d.px, b, 0.0f), pick(w.d.py, b, 0.0f));
    x.q.s = pick(w.d.qs, b, 0.0f);
    x.q.c = pick(w.d.qc, b, 1.0f);
  } else {
    x.p = V(SLDS.spx[b], SLDS.spy[b]);
    x.q.s = 0.0f;  // rot_set(0) == (+0, 1)
    x.q.c = 1.0f;
  }
  return x;
}
HK_DEV v2 body_c(const Arena &w, int b) {
  return b < 3 ? V(pick(w.d.cx, b, 0.0f), pick(w.d.cy, b, 0.0f)) : V(SLDS.spx[b], SLDS.spy[b]);
}
HK_DEV Sweep body_sweep(Arena &w, int b) {
  Sweep s;
  if (b < 3) {
    s.lc = local_center(b);
    s.c0 = V(pick(w.d.c0x, b, 0.0f), pick(w.d.c0y, b, 0.0f));
    s.c = V(pick(w.d.cx, b, 0.0f), pick(w.d.cy, b, 0.0f));
    s.a0 = pick(w.d.a0, b, 0.0f);
    s.a = pick(w.d.a, b, 0.0f);
    s.alpha0 = pick(w.d.al0, b, 0.0f);
  } else {  // static: c0 == c == origin and a0 == a == 0 forever; only alpha0 moves (b2Sweep::Advance)
    s.lc = V(0.0f, 0.0f);
    s.c0 = s.c = V(SLDS.spx[b], SLDS.spy[b]);
    s.a0 = s.a = 0.0f;
    s.alpha0 = LDS(w, kLdsSal0 + b - 3);
  }
  return s;
}
HK_DEV void body_set_sweep(Arena &w, int b, const Sweep &s) {
  if (b < 3) {
    place(w.d.c0x, b, s.c0.x);
    place(w.d.c0y, b, s.c0.y);
    place(w.d.cx, b, s.c.x);
    place(w.d.cy, b, s.c.y);
    place(w.d.a0, b, s.a0);
    place(w.d.a, b, s.a);
    place(w.d.al0, b, s.alpha0);
  } else {
    LDS(w, kLdsSal0 + b - 3) = s.alpha0;
  }
}
// b2Body::SynchronizeTransform
HK_DEV void sync_xf(Arena &w, int b) {
  if (b >= 3) return;  // a static transform is its origin (c - R(0) * 0 == c exactly)
  const float a = pick(w.d.a, b, 0.0f);
  const rot q = rot_set(a);
  const v2 p = vsub(V(pick(w.d.cx, b, 0.0f), pick(w.d.cy, b, 0.0f)), mul_rv(q, local_center(b)));
  place(w.d.qs, b, q.s);
  place(w.d.qc, b, q.c);
  place(w.d.px, b, p.x);
  place(w.d.py, b, p.y);
}
// b2Body::SetAwake (dynamic bodies only; a static body has no awake state that matters here)
HK_DEV void set_awake(Arena &w, int b, int flag) {
  if (b >= 3) return;
  if (flag) {
    if (!pick(w.d.awake, b, 1)) {
      place(w.d.awake, b, 1);
      place(w.d.sleep, b, 0.0f);
    }
  } else {
    place(w.d.awake, b, 0);
    place(w.d.sleep, b, 0.0f);
    place(w.d.vx, b, 0.0f);
    place(w.d.vy, b, 0.0f);
    place(w.d.w, b, 0.0f);
    place(w.d.fx, b, 0.0f);
    place(w.d.fy, b, 0.0f);
    place(w.d.tq, b, 0.0f);
  }
}
// b2Body::Advance
HK_DEV void body_advance(Arena &w, int b, float alpha) {
  Sweep s = body_sweep(w, b);
  sweep_advance(s, alpha);
  s.c = s.c0;
  s.a = s.a0;
  body_set_sweep(w, b, s);
  sync_xf(w, b);
}

// compile-time body helpers (b2Body setters used by the env laws)
template <int B>
HK_DEV void set_transform(Arena &w, v2 p, float angle) {
  const rot q = rot_set(angle);
  w.d.qs[B] = q.s;
  w.d.qc[B] = q.c;
  w.d.px[B] = p.x;
  w.d.py[B] = p.y;
  xform x;
  x.p = p;
  x.q = q;
  const v2 c = mul_xv(x, V(SC.lcx[B], SC.lcy[B]));
  w.d.cx[B] = c.x;
  w.d.cy[B] = c.y;
  w.d.a[B] = angle;
  w.d.c0x[B] = c.x;
  w.d.c0y[B] = c.y;
  w.d.a0[B] = angle;
}
template <int B>
HK_DEV void wake(Arena &w) {
  if (!w.d.awake[B]) { w.d.awake[B] = 1; w.d.sleep[B] = 0.0f; }
}
template <int B>
HK_DEV void set_linear_velocity(Arena &w, v2 v) {
  if (dot(v, v) > 0.0f) wake<B>(w);
  w.d.vx[B] = v.x;
  w.d.vy[B] = v.y;
}
template <int B>
HK_DEV void set_angular_velocity(Arena &w, float om) {
  if (om * om > 0.0f) wake<B>(w);
  w.d.w[B] = om;
}
template <int B>
HK_DEV void apply_force(Arena &w, v2 f) {
  wake<B>(w);
  w.d.fx[B] = w.d.fx[B] + f.x;
  w.d.fy[B] = w.d.fy[B] + f.y;
}
template <int B>
HK_DEV void apply_torque(Arena &w, float t) {
  wake<B>(w);
  w.d.tq[B] += t;
}

}  // namespace hk

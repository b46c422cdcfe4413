// hk_collide.h -- b2ContactManager::Collide: the lane-local broad phase (far tests, interior rectangles),
// ContactDetector.BeginContact, the narrow phase and b2Contact::Update, and the wave's near-pair work list.
#pragma once
#include "hk_body.h"

namespace hk {

// ------------------------------------------------------------------------------------------------
// lane-local broad phase (exact outcome-preserving rejection)
//   Box2D clipping emits points up to sqrt(2) * totalRadius from the reference polygon: reach = 2 * (rA + rB)
//   for polygon pairs; b2CollidePolygonAndCircle and b2TestOverlap need the core distance within rA + rB;
//   every TOI "touching" exit needs the core distance below target + tol < rA + rB at some t.
// ------------------------------------------------------------------------------------------------
HK_DEV float box_gap(float ax0, float ay0, float ax1, float ay1, const float *b) {
  return fmaxf(fmaxf(b[0] - ax1, ax0 - b[2]), fmaxf(b[1] - ay1, ay0 - b[3]));
}
// Axis-aligned box around a player's core (radius-free polygon) relative to its COM at the rotation q:
// {min x, min y, max x, max y} of R(q) (v_i - lc).  Second stage of the far tests below: the bounding disc
// (rcore) is loose for the elongated racket, and a player parked in front of its own goal otherwise sends
// its goal and goal-side wall pairs to the narrow phase / b2TimeOfImpact every step, where they come out
// separated (oracle statistics: ~90 % of b2TimeOfImpact calls).
HK_DEV void player_core_box(const Arena &w, int f, int b, float q_s, float q_c, float (&e)[4],
                            const Scene &S = SC) {
  e[0] = e[1] = kFltMax;
  e[2] = e[3] = -kFltMax;
#pragma unroll
  for (int k = 0; k < kMaxPolyVerts; ++k) {
    if (k < S.fx[f].count) {
      const float ux = S.fx[f].vx[k] - S.lcx[b], uy = S.fx[f].vy[k] - S.lcy[b];
      const float rx = q_c * ux - q_s * uy, ry = q_s * ux + q_c * uy;
      e[0] = fminf(e[0], rx); e[1] = fminf(e[1], ry);
      e[2] = fmaxf(e[2], rx); e[3] = fmaxf(e[3], ry);
    }
  }
}
// both players' core boxes at their current rotations, computed once per pass over the pair table
struct CoreBoxes {
  float e[2][4];
};
HK_DEV void core_boxes(const Arena &w, CoreBoxes &cb) {
  player_core_box(w, F_P1, B_P1, w.d.qs[B_P1], w.d.qc[B_P1], cb.e[0]);
  player_core_box(w, F_P2, B_P2, w.d.qs[B_P2], w.d.qc[B_P2], cb.e[1]);
}
HK_DEV bool static_far_collide(const Scene &S, int fA, int bB, v2 cB, const float (&e)[4], float reach) {
  return box_gap(cB.x + e[0], cB.y + e[1], cB.x + e[2], cB.y + e[3], S.fx_aabb[fA]) > reach;
}
// cb: the players' core boxes when the caller has them (pair-table passes), else computed here
// S: SC for a wave-uniform p (pair-table loops), SLDS for a per-lane p
HK_DEV bool pair_far_collide(const Arena &w, int p, const CoreBoxes *cb = nullptr, const Scene &S = SC) {
  const int fA = S.pairA[p], fB = S.pairB[p], bA = S.pbodyA[p], bB = S.pbodyB[p];
  // A polygon-circle manifold (and a sensor overlap) needs the circle centre within the total radius of
  // the polygon core, so a circle pair is far beyond total + rounding margin; polygon pairs keep the
  // clipping bound 2 * total (+ kFarMargin).
  const float total = S.fx[fA].radius + S.fx[fB].radius;
  const float reach = S.fx[fB].circle ? total + kToiMargin : 2.0f * total + kFarMargin;
  const v2 cB = body_c(w, bB);
  const float rB = S.rcore[bB];
  if (bA >= 3) {
    if (box_gap(cB.x - rB, cB.y - rB, cB.x + rB, cB.y + rB, S.fx_aabb[fA]) > reach) return true;
    if (bB == B_PK) return false;  // a circle's core is its centre: the disc test is already exact
    if (cb) return static_far_collide(S, fA, bB, cB, cb->e[bB == B_P2 ? 1 : 0], reach);
    float e[4];
    player_core_box(w, fB, bB, pick(w.d.qs, bB, 0.0f), pick(w.d.qc, bB, 1.0f), e, S);
    return static_far_collide(S, fA, bB, cB, e, reach);
  }
  const v2 cA = body_c(w, bA);
  const float lim = S.rcore[bA] + rB + reach;
  const float dx = cA.x - cB.x, dy = cA.y - cB.y;
  return dx * dx + dy * dy > lim * lim;
}
// b2TimeOfImpact can only report TOUCHING when the GJK core distance falls below target + tolerance at
// some t.  B's core stays within rcore of its COM, which moves on the segment c0 -> c, so the box gap between
// that swept disc's AABB and A's core AABB bounds the core distance from below: a gap above target +
// tolerance (+ kToiMargin) means alpha = 1 exactly, without running the iteration.
// For a player the second stage bounds its core by the exact box at the end-of-sweep rotation q = rot(a)
// (the transform is synchronised with the sweep whenever the scan runs), widened by rcore * |a - a0|:
// a core point moves at most that far as the angle runs over [a0, a].
// S: SC for a wave-uniform p (first scan pass), SLDS for a per-lane p (later passes)
HK_DEV bool pair_far_toi(const Arena &w, int p, const CoreBoxes &cb, const Scene &S = SC) {  // static A, dynamic B
  const int fA = S.pairA[p], fB = S.pairB[p], bB = S.pbodyB[p];
  // b2TimeOfImpact returns TOUCHING only at a t where the core distance (GJK, or a separation function
  // bounded below by it) is under target + tolerance, target = max(linearSlop, rA + rB - 3 linearSlop),
  // tolerance = linearSlop / 4; every other outcome maps to alpha 1.  A lower bound on the distance above
  // that threshold (+ kToiMargin for rounding) therefore gives alpha 1 exactly.
  const float total = S.fx[fA].radius + S.fx[fB].radius;
  const float reach = fmaxf(kLinearSlop, total - 3.0f * kLinearSlop) + 0.25f * kLinearSlop + kToiMargin;
  const float r = S.rcore[bB];
  const float c0x = pick(w.d.c0x, bB, 0.0f), c0y = pick(w.d.c0y, bB, 0.0f);
  const float cx = pick(w.d.cx, bB, 0.0f), cy = pick(w.d.cy, bB, 0.0f);
  const float lx = fminf(c0x, cx), ly = fminf(c0y, cy), hx = fmaxf(c0x, cx), hy = fmaxf(c0y, cy);
  if (box_gap(lx - r, ly - r, hx + r, hy + r, S.fx_aabb[fA]) > reach) return true;
  if (bB == B_PK) return false;  // circle: exact already
  const float(&e)[4] = cb.e[bB == B_P2 ? 1 : 0];
  const float rot = r * fabsf(pick(w.d.a, bB, 0.0f) - pick(w.d.a0, bB, 0.0f));
  return box_gap(lx + e[0] - rot, ly + e[1] - rot, hx + e[2] + rot, hy + e[3] + rot, S.fx_aabb[fA]) > reach;
}

// First-pass bulk settlement of the TOI scan (solve_toi).  A dynamic body whose swept core box lies inside its
// interior rectangle is farther than the TOI reach from each of its static fixtures (walls bound the
// rectangle in y, posts and goals in x), so pair_far_toi holds for all of its TOI pairs.  The rectangles are
// compile-time (1 mm inside the exact bound); the static_asserts re-check every fixture against them.
struct Rect { float x0, y0, x1, y1; };
constexpr float cmax(float a, float b) { return a > b ? a : b; }
constexpr float cmin(float a, float b) { return a < b ? a : b; }
constexpr float toi_reach(int fB) {
  const float total = g_scene.fx[F_WT].radius + g_scene.fx[fB].radius;
  return cmax(kLinearSlop, total - 3.0f * kLinearSlop) + 0.25f * kLinearSlop + kToiMargin;
}
constexpr Rect interior_rect(int fB, bool goals) {
  const float e = toi_reach(fB) + 1e-3f;
  float xl = cmax(g_scene.fx_aabb[F_PLT][2], g_scene.fx_aabb[F_PLB][2]);
  float xr = cmin(g_scene.fx_aabb[F_PRT][0], g_scene.fx_aabb[F_PRB][0]);
  if (goals) {
    xl = cmax(xl, g_scene.fx_aabb[F_G1][2]);
    xr = cmin(xr, g_scene.fx_aabb[F_G2][0]);
  }
  return Rect{xl + e, g_scene.fx_aabb[F_WB][3] + e, xr - e, g_scene.fx_aabb[F_WT][1] - e};
}
constexpr Rect kInteriorPuck = interior_rect(F_PK, false), kInteriorPlayer = interior_rect(F_P1, true);
constexpr bool rect_clear(const Rect &r, int f, float reach) {
  const float *b = g_scene.fx_aabb[f];
  return cmax(cmax(b[0] - r.x1, r.x0 - b[2]), cmax(b[1] - r.y1, r.y0 - b[3])) > reach;
}
constexpr bool interior_ok() {
  const int fs[8] = {F_WT, F_WB, F_PLT, F_PLB, F_PRT, F_PRB, F_G1, F_G2};
  bool ok = g_scene.fx[F_P1].radius == g_scene.fx[F_P2].radius;
  for (int k = 0; k < 8; ++k) ok = ok && rect_clear(kInteriorPlayer, fs[k], toi_reach(F_P1));
  for (int k = 0; k < 6; ++k) ok = ok && rect_clear(kInteriorPuck, fs[k], toi_reach(F_PK));
  for (int p = 0; p < NP; ++p)  // the puck's TOI pairs are 0..5, the players' their static pairs (kEdgeMask)
    if ((kToiPairs >> p) & 1u) {
      const int f = g_scene.pairA[p];
      const bool known = f == F_WT || f == F_WB || f == F_PLT || f == F_PLB || f == F_PRT || f == F_PRB ||
                         (g_scene.pbodyB[p] != B_PK && (f == F_G1 || f == F_G2));
      ok = ok && known;
    }
  return ok;
}
static_assert(interior_ok(), "interior rectangles clear every static fixture of a TOI pair by the TOI reach");
HK_DEV bool inside(const Rect &r, float lx, float ly, float hx, float hy) {
  return lx > r.x0 && ly > r.y0 && hx < r.x1 && hy < r.y1;
}

// ------------------------------------------------------------------------------------------------
// ContactDetector.BeginContact (hockey_env.py:44-76) and b2Contact::Update
// ------------------------------------------------------------------------------------------------
HK_DEV void begin_contact(Arena &w, int p) {  // per-lane p
  const int bA = SLDS.pbodyA[p], bB = SLDS.pbodyB[p];
  const int hasPK = (bA == B_PK || bB == B_PK);
  if ((bA == B_G2 || bB == B_G2) && hasPK) { w.done = 1; w.winner = 1; }
  if ((bA == B_G1 || bB == B_G1) && hasPK) { w.done = 1; w.winner = -1; }
  if ((bA == B_P1 || bB == B_P1) && hasPK) {
    if (w.keep_mode && (double)w.d.vx[B_PK] < 0.1)
      if (w.has1 == 0) w.has1 = 15;
  }
  if ((bA == B_P2 || bB == B_P2) && hasPK) {
    if (w.keep_mode && (double)w.d.vx[B_PK] > -0.1)
      if (w.has2 == 0) w.has2 = 15;
  }
}

// Narrow phase of pair p for the arena whose manifold records start at `man` (arena index a of n): the
// manifold from the two fixtures' transforms, the impulse carry-over from the stored manifold (ids matched,
// meaningful only if the pair was touching), and the whole-record write when touching.  Returns touching.
// Reads only its arguments, the scene and the pair's own record, so any lane may run it for any arena.
HK_DEV int narrow_phase(float *man, int64_t n, int64_t a, int p, int was, const xform &xA, const xform &xB) {
  const int fA = SLDS.pairA[p], fB = SLDS.pairB[p], bA = SLDS.pbodyA[p];
  // the stored manifold (ids / impulses) of a touching pair is requested before the narrow phase so its
  // HBM / L2 latency overlaps the clipping arithmetic
  const int slot = SLDS.manslot[p];
  Quad *rec = reinterpret_cast<Quad *>(man + ((int64_t)(slot < 0 ? 0 : slot) * n + a) * NMF);
  Quad o0 = Quad{0.0f, 0.0f, 0.0f, 0.0f}, o2 = o0, o3 = o0;
  if (slot >= 0 && was) {
    o0 = rec[0];
    o2 = rec[2];
    o3 = rec[3];
  }
  if (SLDS.sensor[p]) return test_overlap(SLDS.fx[fA], xA, SLDS.fx[fB], xB);
  Manifold m;
  if (SLDS.fx[fB].circle) {  // puck: A is a static quad or a player
    const RFix<1> cB = load_fix<1>(SLDS.fx[fB]);
    if (bA >= 3) collide_poly_circle(m, load_fix<kStaticVerts>(SLDS.fx[fA]), xA, cB, xB);
    else collide_poly_circle(m, load_fix<kMaxPolyVerts>(SLDS.fx[fA]), xA, cB, xB);
  } else {  // player B: A is a static quad or the other player
    const RFix<kMaxPolyVerts> pB = load_fix<kMaxPolyVerts>(SLDS.fx[fB]);
    if (bA >= 3) collide_polygons(m, load_fix<kStaticVerts>(SLDS.fx[fA]), xA, pB, xB);
    else collide_polygons(m, load_fix<kMaxPolyVerts>(SLDS.fx[fA]), xA, pB, xB);
  }
  const int touching = m.count > 0;
  if (touching) {
    // match old contact ids to carry impulses (the stored manifold is meaningful only if touching)
    int oc = 0;
    uint32_t oid0 = 0u, oid1 = 0u;
    float oni0 = 0.0f, oni1 = 0.0f, oti0 = 0.0f, oti1 = 0.0f;
    if (was) {
      oc = __float_as_int(o0.x) & 0xff;
      oid0 = (uint32_t)__float_as_int(o2.y);
      oid1 = (uint32_t)__float_as_int(o2.z);
      oni0 = o3.x;
      oti0 = o3.y;
      oni1 = o3.z;
      oti1 = o3.w;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i < m.count) {
        m.ni[i] = 0.0f;
        m.ti[i] = 0.0f;
        if (oc > 0 && oid0 == m.id[i]) { m.ni[i] = oni0; m.ti[i] = oti0; }
        else if (oc > 1 && oid1 == m.id[i]) { m.ni[i] = oni1; m.ti[i] = oti1; }
      }
    }
    // whole-record write; a one-point manifold's point-1 words are zeroed (every reader is bounded by
    // the point count, as in Box2D)
    const bool two = m.count > 1;
    rec[0] = Quad{__int_as_float(m.count | (m.type << 8)), m.ln.x, m.ln.y, m.lp.x};
    rec[1] = Quad{m.lp.y, m.pt_lp[0].x, m.pt_lp[0].y, two ? m.pt_lp[1].x : 0.0f};
    rec[2] = Quad{two ? m.pt_lp[1].y : 0.0f, __int_as_float((int)m.id[0]), two ? __int_as_float((int)m.id[1]) : 0,
                  0.0f};
    rec[3] = Quad{m.ni[0], m.ti[0], two ? m.ni[1] : 0.0f, two ? m.ti[1] : 0.0f};
  }
  return touching;
}

// b2Contact::Update bookkeeping of pair p once its narrow phase has run: enable, wake-ups on a touching
// change (solid pairs), the touching bit and BeginContact -- the order-dependent side effects, applied by the
// owner lane in pair order.
HK_DEV void pair_update_apply(Arena &w, int p, int touching) {
  const uint32_t bit = 1u << p;
  const int was = (w.touch & bit) != 0u;
  w.enabled |= bit;
  if (!SLDS.sensor[p] && touching != was) { set_awake(w, SLDS.pbodyA[p], 1); set_awake(w, SLDS.pbodyB[p], 1); }
  w.touch = touching ? (w.touch | bit) : (w.touch & ~bit);
  if (!was && touching) begin_contact(w, p);
}

// b2Contact::Update for a pair the broad phase could not reject: narrow phase, impulse carry-over,
// wake-ups and BeginContact.
HK_DEV void pair_update_near(Arena &w, int p) {
  const int was = (w.touch & (1u << p)) != 0u;
  const int touching = narrow_phase(w.man, w.n, w.a, p, was, body_xf(w, SLDS.pbodyA[p]), body_xf(w, SLDS.pbodyB[p]));
  pair_update_apply(w, p, touching);
}

// b2Contact::Update for a pair the broad phase rejects: not touching (no manifold, no BeginContact)
HK_DEV void pair_update_far(Arena &w, int p, const Scene &S = SC) {
  const uint32_t bit = 1u << p;
  const int was = (w.touch & bit) != 0u;
  w.enabled |= bit;
  if (!S.sensor[p] && was) { set_awake(w, S.pbodyA[p], 1); set_awake(w, S.pbodyB[p], 1); }
  w.touch &= ~bit;
}

HK_DEV void pair_update(Arena &w, int p) {  // per-lane p (TOI events)
  if (pair_far_collide(w, p, nullptr, SLDS)) pair_update_far(w, p, SLDS);
  else pair_update_near(w, p);
}

// The near pairs' narrow phases of the whole wave, dealt out over all its lanes (device build; every lane of
// the wave that runs the step calls it).  Per lane, `near` holds the pairs whose narrow phase must run.  With
// every dynamic body awake the narrow phases of one lane are independent of each other (transforms do not
// change during Collide, wake-ups of awake bodies are no-ops, BeginContact touches no narrow-phase input), so
// they may run anywhere and in any order: each (lane, pair) goes to an LDS work list with the pair's two body
// transforms, a worker lane runs narrow_phase for the owner's arena (reading and writing the owner's manifold
// record in HBM) and leaves `touching` in the owner's LDS row; the owner then applies the order-dependent
// bookkeeping in pair order.  A lane with k near pairs no longer holds the wave for k narrow phases.
HK_DEV void collide_near_wave(Arena &w, uint32_t near) {
#if defined(__HIP_DEVICE_COMPILE__)
  float *q = w.lds + kLdsPerLane * 64;
  const uint64_t lt = (1ull << w.lane) - 1ull;
  const int64_t a0 = w.a - w.lane;  // arena of lane 0 of this wave
  while (wave_any(near != 0u)) {
    const int cnt = __popc(near);
    int off = 0, total = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      const uint64_t m = __ballot((cnt >> b) & 1);
      off += __popcll(m & lt) << b;
      total += __popcll(m) << b;
    }
    uint32_t listed = 0u;
    for (uint32_t m = near; m && off < kToiQ; m &= m - 1u, ++off) {
      const int p = __ffs(m) - 1;
      const xform xA = body_xf(w, SLDS.pbodyA[p]), xB = body_xf(w, SLDS.pbodyB[p]);
      const int was = (w.touch >> p) & 1u;
      float *it = q + off * kToiItemWords;
      it[0] = __int_as_float(p | (w.lane << 8) | (was << 16));
      it[1] = xA.p.x;
      it[2] = xA.p.y;
      it[3] = xA.q.s;
      it[4] = xA.q.c;
      it[5] = xB.p.x;
      it[6] = xB.p.y;
      it[7] = xB.q.s;
      it[8] = xB.q.c;
      listed |= m & (0u - m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n = total < kToiQ ? total : kToiQ;
    const uint64_t act = __ballot(1);  // workers: the wave's active lanes (see toi_drain_wave)
    const int rank = __popcll(act & lt), nact = __popcll(act);
    for (int k = rank; k < n; k += nact) {
      const float *it = q + k * kToiItemWords;
      const int tag = __float_as_int(it[0]), p = tag & 255, owner = (tag >> 8) & 255, was = (tag >> 16) & 1;
      xform xA, xB;
      xA.p = V(it[1], it[2]);
      xA.q.s = it[3];
      xA.q.c = it[4];
      xB.p = V(it[5], it[6]);
      xB.q.s = it[7];
      xB.q.c = it[8];
      const int touching = narrow_phase(w.man, w.n, a0 + owner, p, was, xA, xB);
      w.lds[(kLdsToi + p) * 64 + owner] = touching ? 1.0f : 0.0f;  // the TOI cache row is free until SolveTOI
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    near &= ~listed;
    for (uint32_t m = listed; m; m &= m - 1u) {  // pair order
      const int p = __ffs(m) - 1;
      pair_update_apply(w, p, LDS(w, kLdsToi + p) != 0.0f);
    }
  }
#else  // host build (one lane at a time): the lane's own queue in pair order
  while (near) {
    const int p = __ffs(near) - 1;
    near &= near - 1u;
    pair_update_near(w, p);
  }
#endif
}

// b2ContactManager::Collide.  With every dynamic body awake (the normal state of play: no arena-step of a
// strong-vs-strong run has a sleeping body) the pair order only matters among pairs that can touch
// (wake-ups are no-ops, far pairs fire no BeginContact), so the far pairs are settled first and the near
// pairs' narrow phases are dealt out over the wave (collide_near_wave).  A lane with a sleeping body takes
// Box2D's sequential loop afterwards.
HK_DEV void collide(Arena &w) {
  const bool fast = w.d.awake[0] && w.d.awake[1] && w.d.awake[2];
  uint32_t near = 0u;
  if (fast) {
    CoreBoxes cb;
    core_boxes(w, cb);
#pragma unroll
    for (int p = 0; p < NP; ++p) {  // uniform loop, unrolled: the scene data are literals
      if (pair_far_collide(w, p, &cb)) pair_update_far(w, p);
      else near |= 1u << p;
    }
  }
  collide_near_wave(w, near);  // every lane (a lane on the sequential path contributes worker capacity)
  if (fast) return;
  for (int p = 0; p < NP; ++p) {
    const int bA = SC.pbodyA[p], bB = SC.pbodyB[p];
    const int activeA = bA < 3 && pick(w.d.awake, bA, 0);
    const int activeB = pick(w.d.awake, bB, 0);
    if (!activeA && !activeB) continue;
    pair_update(w, p);
  }
}

}  // namespace hk

// hk_world.h -- b2World::Step: Solve (islands), SolveTOI (scan, cooperative b2TimeOfImpact drain, TOI events) and
// ClearForces, on the contact solver of hk_solver.h / hk_velocity.h.
#pragma once
#include "hk_collide.h"
#include "hk_solver.h"

namespace hk {

// ------------------------------------------------------------------------------------------------
// b2World::Solve: islands by DFS (Box2D's seed order and edge order), solved together (they share no
// dynamic body), position early exit and sleep per island.
// ------------------------------------------------------------------------------------------------
template <typename SL>
HK_DEV bool solve_islands(Arena &w, SL &S, float dt, PhaseT &T) {
  constexpr int MAXS = SlotCap<SL>::value;
  const float h = dt;
  int island_of[3] = {-1, -1, -1};
  int nc = 0, nisl = 0;
  uint32_t inis = 0u;
  const uint32_t live = w.enabled & w.touch & ~kSensorMask;
  const int seed_order[3] = {B_PK, B_P2, B_P1};
#pragma unroll
  for (int si = 0; si < 3; ++si) {
    const int seed = seed_order[si];
    if (island_of[seed] >= 0 || !w.d.awake[seed]) continue;
    const int isl = nisl++;
    int st0 = seed, st1 = 0, st2 = 0, sc = 1;  // DFS stack of dynamic bodies (statics never propagate)
    island_of[seed] = isl;
    while (sc > 0) {
      const int bi = sc == 3 ? st2 : (sc == 2 ? st1 : st0);
      --sc;
      set_awake(w, bi, 1);
      uint32_t m = pick(kEdgeMask, bi, 0u) & live & ~inis;
      while (m) {
        const int e = __ffs(m) - 1;
        m &= m - 1u;
        inis |= 1u << e;
        S.set_pair(nc, e, isl);
        ++nc;
        const int pa = SLDS.pbodyA[e], pb = SLDS.pbodyB[e];
        const int other = pa == bi ? pb : pa;
        if (other >= 3) continue;
        if (pick(island_of, other, 0) >= 0) continue;
        place(island_of, other, isl);
        if (sc == 0) st0 = other; else if (sc == 1) st1 = other; else st2 = other;
        ++sc;
      }
    }
  }
  if (nc > MAXS) return false;
  // integrate velocities (b2Island::Solve), in place in the register body file
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    if (island_of[b] >= 0) {
      w.d.c0x[b] = w.d.cx[b];
      w.d.c0y[b] = w.d.cy[b];
      w.d.a0[b] = w.d.a[b];
      v2 v = V(w.d.vx[b], w.d.vy[b]);
      float wv = w.d.w[b];
      v = vadd(v, vs(h, vadd(vs(1.0f, V(0.0f, 0.0f)), vs(SC.invMass[b], V(w.d.fx[b], w.d.fy[b])))));
      wv += h * SC.invI[b] * w.d.tq[b];
      v = vs(1.0f / (1.0f + h * w.d.ld[b]), v);
      wv *= 1.0f / (1.0f + h * w.d.ad[b]);
      w.d.vx[b] = v.x;
      w.d.vy[b] = v.y;
      w.d.w[b] = wv;
    }
  }
  HK_TRACE_POINT(w, 3);
  S.each(nc, [&](FSlot &s, int) {
    fslot_load(s, w, fs_pair(s), 1, fs_isl(s));
    fslot_init_velocity(s, w);
  });
  S.each(nc, [&](FSlot &s, int) { fslot_warm_start(s, w.d); });
  HK_TIC(T, 2);  // diagnostics: island setup (DFS, integrate, constraint init, warm start)
  const int vit = velocity_iterations(S, w.d, nc, island_of, T);
  HK_TIC(T, 3);  // diagnostics: velocity iterations
#ifdef HK_PHASE_TIMERS
  w.dg_vit_isl += vit;
  w.dg_nc_max = nc > w.dg_nc_max ? nc : w.dg_nc_max;
#endif
  (void)vit;
  S.each(nc, [&](FSlot &s, int) { fslot_store(s, w); });
#pragma unroll
  for (int b = 0; b < 3; ++b)
    if (island_of[b] >= 0) integrate_one(h, w.d, b);
  int solved = 0;
  const int all = (1 << nisl) - 1;
  S.load_geo(nc, w);
  for (int it = 0; it < kPosIters && (solved & all) != all; ++it) {
    HK_MARK(pos_begin);
    float ms0 = 0.0f, ms1 = 0.0f, ms2 = 0.0f;
    S.each(nc, [&](FSlot &s, int i) {
      const int isl = fs_isl(s);
      if (!((solved >> isl) & 1)) {
        const float m = fslot_solve_position(s, w, kBaumgarte, 0.0f, S.geo(i, s, w));
        ms0 = isl == 0 ? fmin2(ms0, m) : ms0;
        ms1 = isl == 1 ? fmin2(ms1, m) : ms1;
        ms2 = isl == 2 ? fmin2(ms2, m) : ms2;
      }
    });
#ifdef HK_PHASE_TIMERS
    w.dg_pit++;
#endif
    if (ms0 >= -3.0f * kLinearSlop) solved |= 1;
    if (ms1 >= -3.0f * kLinearSlop) solved |= 2;
    if (ms2 >= -3.0f * kLinearSlop) solved |= 4;
    HK_MARK(pos_end);
  }
#pragma unroll
  for (int b = 0; b < 3; ++b)
    if (island_of[b] >= 0) sync_xf(w, b);
  const float linTolSqr = kLinearSleepTol * kLinearSleepTol;
  const float angTolSqr = kAngularSleepTol * kAngularSleepTol;
  for (int isl = 0; isl < nisl; ++isl) {
    float minSleep = kFltMax;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (island_of[b] == isl) {
        if (w.d.w[b] * w.d.w[b] > angTolSqr || w.d.vx[b] * w.d.vx[b] + w.d.vy[b] * w.d.vy[b] > linTolSqr) {
          w.d.sleep[b] = 0.0f;
          minSleep = 0.0f;
        } else {
          w.d.sleep[b] += h;
          minSleep = fmin2(minSleep, w.d.sleep[b]);
        }
      }
    }
    if (minSleep >= kTimeToSleep && ((solved >> isl) & 1)) {
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if (island_of[b] == isl) set_awake(w, b, 0);
    }
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// b2World::SolveTOI.  In this scene a TOI pair is always (static A, dynamic B), so the mini-island
// holds exactly one dynamic body: B plus its touching static contacts (minContact first, then B's
// contact edges in order).  Mass gating of SolveTOIPositionConstraints is therefore the identity.
// ------------------------------------------------------------------------------------------------
template <typename SL>
HK_DEV void toi_island_solve(Arena &w, SL &S, int minc, uint32_t extra, int nc, int db, float sub_dt, PhaseT &T) {
  uint32_t m = extra;
  S.each(nc, [&](FSlot &s, int i) {
    int p = minc;
    if (i > 0) { p = __ffs(m) - 1; m &= m - 1u; }
    fslot_load(s, w, p, 0, 0);
  });
  for (int it = 0; it < 20; ++it) {
    float minSep = 0.0f;
    S.each(nc, [&](FSlot &s, int i) {
      // geometry re-read per pass here: caching it in the slot file miscompiles on gfx950 in this loop
      // (ROCm 7.2; caught by the GPU lockstep tests), and TOI position passes are few
      minSep = fslot_solve_position(s, w, kToiBaumgarte, minSep, man_geo(w, fs_pair(s)));
    });
    if (minSep >= -1.5f * kLinearSlop) break;
  }
  HK_TIC(T, 10);  // diagnostics: TOI position passes
  // leap of faith (the static body's c0 already equals its c)
  place(w.d.c0x, db, pick(w.d.cx, db, 0.0f));
  place(w.d.c0y, db, pick(w.d.cy, db, 0.0f));
  place(w.d.a0, db, pick(w.d.a, db, 0.0f));
  S.each(nc, [&](FSlot &s, int) { fslot_init_velocity(s, w); });
  const int isl_of[3] = {db == 0 ? 0 : -1, db == 1 ? 0 : -1, db == 2 ? 0 : -1};  // one island: B
  const int vit = velocity_iterations(S, w.d, nc, isl_of, T);
  HK_TIC(T, 11);  // diagnostics: TOI velocity iterations
#ifdef HK_PHASE_TIMERS
  w.dg_vit_toi += vit;
#endif
  (void)vit;
#pragma unroll
  for (int b = 0; b < 3; ++b)
    if (b == db) integrate_one(sub_dt, w.d, b);
  sync_xf(w, db);
}

// The lean event path: a mini-island of ONE contact (99.7 % of TOI events, hk_body.h) between static body A and
// dynamic body B = db, for the lanes of a round that hold one (the per-lane test in solve_toi).  It runs
// toi_island_solve's float operations in toi_island_solve's order, for the values that path has in this case:
//   * the manifold geometry is read once per event and serves the slot's meta word, every position pass and
//     InitializeVelocityConstraints (the generic path reads the record 2 + passes times);
//   * body A is static: its centre is the scene origin, its rotation (+0, 1), its inverse mass and inertia +0 (what
//     inv_mass / inv_inertia / get_pos_a return for it), so nothing of A is gathered, tested or written; the
//     arithmetic on A's centre is kept in a local as written (cA - 0 * P), so a non-finite impulse spreads as it does
//     in fslot_solve_position;
//   * body B's centre and angle stay in locals over the position passes and are written back once, with the leap
//     of faith (c0 = c, a0 = a);
//   * one constraint set-up, then the one-contact velocity family's static-body-A arms directly
//     (vone_family_static_a): what velocity_iterations dispatches to for a wave of such lanes (first comparison at
//     iteration 7, no slot swap), with the same vone_chunk arms, the 180-iteration cap, the period-4 exit and
//     chunk_end, on body B's velocity in locals.
template <int kType>
HK_DEV float toi_one_position_pass(const ManGeo &m, int pcount, f2 &cA, f2 &cB, float &aB, f2 lcB, float mB, float iB,
                                   float rBr) {
  const float mA = 0.0f, iA = 0.0f, rAr = pair_rA();
  const f2 lcA = f2{0.0f, 0.0f};
  const f2 ln = F2(m.ln), lp = F2(m.lp);
  float minSep = 0.0f;
  HK_EV(EV_POS_PT, pcount);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < pcount) {
      rot qA, qB;
      qA.s = 0.0f;  // rot_set(+0) == (+0, 1)
      qA.c = 1.0f;
      qB = rot_set(aB);
      const f2 pA = cA - prv(qA, lcA), pB = cB - prv(qB, lcB);
      f2 normal, point;
      float sep;
      if constexpr (kType == 1) {
        normal = prv(qA, ln);
        const f2 plane = prv(qA, lp) + pA;
        const f2 clip = prv(qB, F2(m.pt[j])) + pB;
        sep = pdot(clip - plane, normal) - rAr - rBr;
        point = clip;
      } else {
        normal = prv(qB, ln);
        const f2 plane = prv(qB, lp) + pB;
        const f2 clip = prv(qA, F2(m.pt[j])) + pA;
        sep = pdot(clip - plane, normal) - rAr - rBr;
        point = clip;
        normal = -normal;
      }
      const f2 rA = point - cA, rB = point - cB;
      minSep = fmin2(minSep, sep);
      float C = fclamp(kToiBaumgarte * (sep + kLinearSlop), -kMaxLinearCorrection, 0.0f);
      float rnA = pcrs(rA, normal), rnB = pcrs(rB, normal);
      float K = mA + mB + iA * rnA * rnA + iB * rnB * rnB;
      float impulse = K > 0.0f ? -C / K : 0.0f;
      const f2 P = bc(impulse) * normal;
      cA = cA - bc(mA) * P;
      cB = cB + bc(mB) * P;
      aB += iB * pcrs(rB, P);
    }
  }
  return minSep;
}
HK_DEV void toi_island_solve_one(Arena &w, int minc, int bA, int db, float sub_dt, PhaseT &T) {
  HK_HOST_TOI_LEAN_INC();
#ifdef HK_PHASE_TIMERS
  w.dg_toi_lean++;
#endif
  HK_MARK(toi_lean_begin);
  const ManGeo m = man_geo(w, minc);
  FSlot s;
  fslot_load(s, w, minc, 0, 0, &m);
  {
    const int pcount = fs_pcount(s);
    const f2 lcB = F2(local_center(db));
    const float mB = s.mB, iB = s.iB, rBr = pair_rB(db);
    const f2 cA0 = f2{SLDS.spx[bA], SLDS.spy[bA]};
    v2 c0;
    float aB;
    get_pos_b(w.d, db, c0, aB);
    f2 cB = F2(c0);
    // the manifold type is the event's: each type's passes are a loop of their own
    const auto passes = [&](auto kType) {
      for (int it = 0; it < 20; ++it) {
        f2 cA = cA0;  // a static body's centre is not written back: every pass starts from the scene's
        const float minSep = toi_one_position_pass<decltype(kType)::value>(m, pcount, cA, cB, aB, lcB, mB, iB, rBr);
        if (minSep >= -1.5f * kLinearSlop) break;
      }
    };
    if (m.type == 1) passes(kint<1>{});
    else passes(kint<2>{});
    HK_MARK(toi_lean_pos_end);
    HK_TIC(T, 16);  // diagnostics: TOI position passes, lean path
    // body B back to the body file together with the leap of faith (c0 = c, a0 = a)
    place(w.d.cx, db, cB[0]);
    place(w.d.cy, db, cB[1]);
    place(w.d.a, db, aB);
    place(w.d.c0x, db, cB[0]);
    place(w.d.c0y, db, cB[1]);
    place(w.d.a0, db, aB);
  }
  fslot_init_velocity(s, w, &m);
  HK_MARK(toi_lean_vel_begin);
  v2 vB2;
  float wB;
  get_vel_b(w.d, db, vB2, wB);
  f2 vB = F2(vB2);
  HK_FAM_T0();
  const int it = vone_family_static_a(s, vB, wB);
  HK_FAM_ADD(T, 2);
  set_vel_b(w.d, db, V2(vB), wB);
  HK_TIC(T, 17);  // diagnostics: TOI velocity iterations, lean path
#ifdef HK_PHASE_TIMERS
  w.dg_vit_toi += it;
#endif
  (void)it;
#pragma unroll
  for (int b = 0; b < 3; ++b)
    if (b == db) integrate_one(sub_dt, w.d, b);
  sync_xf(w, db);
  HK_MARK(toi_lean_end);
}

// b2TimeOfImpact of static-vs-dynamic pair p from the two sweeps -> alpha in the step's [alpha0, 1] frame
// (sB.alpha0 == max(alpha0 A, alpha0 B) after alignment)
HK_DEV float toi_pair_sweeps(int p, const Sweep &sA, const Sweep &sB) {
  const Proxy<kStaticVerts, true> pA = make_proxy<kStaticVerts, true>(SLDS.fx[SLDS.pairA[p]]);
  const Proxy<kMaxPolyVerts> pB = make_proxy<kMaxPolyVerts>(SLDS.fx[SLDS.pairB[p]]);
  float beta;
  const int st = time_of_impact(pA, pB, sA, sB, 1.0f, beta);
  return st == TOI_TOUCHING ? fmin2(sB.alpha0 + (1.0f - sB.alpha0) * beta, 1.0f) : 1.0f;
}
// per-lane pair p of this lane's arena
HK_DEV float toi_pair(Arena &w, int p) {
#ifdef HK_PHASE_TIMERS
  w.dg_toi_calls++;
#endif
  return toi_pair_sweeps(p, body_sweep(w, SLDS.pbodyA[p]), body_sweep(w, SLDS.pbodyB[p]));
}
// runs the lane's queued b2TimeOfImpact calls in pair order; `below` tracks the pairs whose cached alpha is
// below 1 (the only ones the minimum selection can pick: it starts at 1 and compares strictly)
HK_DEV void toi_drain(Arena &w, uint32_t &pending, uint32_t &below) {
  while (pending) {
    const int p = __ffs(pending) - 1;
    pending &= pending - 1u;
    float alpha = toi_pair(w, p);
    LDS(w, kLdsToi + p) = alpha;
    below = alpha < 1.0f ? (below | (1u << p)) : (below & ~(1u << p));
  }
}

// Cooperative drain (device build; every lane of the wave that runs the step calls it, with or without queued
// pairs).  A per-lane queue holds the wave for as many rounds as its longest queue; here the wave's queued
// (lane, pair) calls are listed in LDS -- pair id, owner lane and the two sweeps' inputs, copied at this point
// -- and dealt out to all lanes, so a lane with k queued pairs no longer costs k rounds.  A worker writes alpha
// into the owner's TOI cache slot; the owner then updates `below`.  The calls are independent (each reads only
// its own pair's sweeps, which nothing changes until the drain is over), and a worker runs the same arithmetic
// on the same inputs as the owner would: bit-identical alphas.  The host build (one lane at a time) drains per
// lane.
HK_DEV void toi_drain_wave(Arena &w, uint32_t &pending, uint32_t &below) {
#if defined(__HIP_DEVICE_COMPILE__)
  float *q = w.lds + kLdsPerLane * 64;
  const uint64_t lt = (1ull << w.lane) - 1ull;  // lanes below this one
  while (wave_any(pending != 0u)) {
    // exclusive prefix sum of the lanes' queue lengths (<= 27: five bit-planes of ballots)
    const int cnt = __popc(pending);
    int off = 0, total = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      const uint64_t m = __ballot((cnt >> b) & 1);
      off += __popcll(m & lt) << b;
      total += __popcll(m) << b;
    }
    uint32_t listed = 0u;
    for (uint32_t m = pending; m && off < kToiQ; m &= m - 1u, ++off) {
      const int p = __ffs(m) - 1;
      const Sweep sB = body_sweep(w, SLDS.pbodyB[p]);
      float *it = q + off * kToiItemWords;
      it[0] = __int_as_float(p | (w.lane << 8));
      it[1] = sB.c0.x;
      it[2] = sB.c0.y;
      it[3] = sB.c.x;
      it[4] = sB.c.y;
      it[5] = sB.a0;
      it[6] = sB.a;
      it[7] = sB.alpha0;
      it[8] = LDS(w, kLdsSal0 + SLDS.pbodyA[p] - 3);  // the static body's alpha0
      listed |= m & (0u - m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n = total < kToiQ ? total : kToiQ;
    // the workers are the wave's ACTIVE lanes (a partial last wave, or a single-arena context, has fewer
    // than 64): active lane r takes items r, r + nact, ...
    const uint64_t act = __ballot(1);
    const int rank = __popcll(act & lt), nact = __popcll(act);
    for (int k = rank; k < n; k += nact) {
      const float *it = q + k * kToiItemWords;
      const int tag = __float_as_int(it[0]), p = tag & 255, owner = tag >> 8;
      const int bA = SLDS.pbodyA[p], bB = SLDS.pbodyB[p];
      Sweep sA, sB;
      sA.lc = V(0.0f, 0.0f);
      sA.c0 = sA.c = V(SLDS.spx[bA], SLDS.spy[bA]);
      sA.a0 = sA.a = 0.0f;
      sA.alpha0 = it[8];
      sB.lc = local_center(bB);
      sB.c0 = V(it[1], it[2]);
      sB.c = V(it[3], it[4]);
      sB.a0 = it[5];
      sB.a = it[6];
      sB.alpha0 = it[7];
      w.lds[(kLdsToi + p) * 64 + owner] = toi_pair_sweeps(p, sA, sB);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#ifdef HK_PHASE_TIMERS
    w.dg_toi_calls += __popc(listed);
#endif
    pending &= ~listed;
    for (uint32_t m = listed; m; m &= m - 1u) {
      const int p = __ffs(m) - 1;
      const float alpha = LDS(w, kLdsToi + p);
      below = alpha < 1.0f ? (below | (1u << p)) : (below & ~(1u << p));
    }
  }
#else
  toi_drain(w, pending, below);
#endif
}

HK_DEV void solve_toi(Arena &w, float dt, PhaseT &T) {
#pragma unroll
  for (int b = 0; b < 3; ++b) w.d.al0[b] = 0.0f;
  for (int k = 0; k < 8; ++k) LDS(w, kLdsSal0 + k) = 0.0f;
  for (int p = 0; p < NP; ++p) LDS(w, kLdsCnt + p) = 0.0f;  // TOI alphas: only read below 1 (`below`)
  w.toiflag = 0u;
  w.cisl = 0u;
  w.bisl = 0u;
  uint32_t below = 0u;      // pairs whose cached TOI alpha (LDS) is < 1
  uint32_t exhausted = 0u;  // pairs past b2_maxSubSteps TOI events this step (toi_count > 8, kept in LDS)
  uint32_t redo = 0u;       // pairs a later scan pass must visit: the last event's body's contacts
  bool first = true;
  // The lanes stay together in this loop until every lane is done (`act`), so that the b2TimeOfImpact calls
  // of step (2) can be dealt out over the whole wave (toi_drain_wave).  A lane that is done only contributes
  // worker capacity.
  bool act = true;
  while (wave_any(act)) {
    HK_TIC(T, 5);  // diagnostics: events / min selection -> "toi-events"
    uint32_t elig = 0u, pending = 0u;
    if (act) {
      // (1) In pair order: eligibility, sweep alignment (the only order-dependent side effect) and the cheap
      //     far rejection.  Pairs that need a real b2TimeOfImpact are queued.  During a step the alignment
      //     only ever advances a STATIC body's alpha0 (TOI events come in non-decreasing alpha, and only the
      //     moved body's pairs are re-evaluated, so a0(static) <= a0(dynamic) for them); the queued TOIs
      //     therefore see exactly the sweeps the sequential scan would.  Should a dynamic body ever be
      //     advanced here, its lane first drains its queue so the sequential order is kept regardless.
      CoreBoxes cb;  // the players' poses are fixed during the pass (only sweep starts move)
      core_boxes(w, cb);
      uint32_t todo;
      if (first) {
        uint32_t settled = 0u;
        // The first pass has no order-dependent side effect (every alpha0 is still 0, so the alignment is a
        // no-op): the TOI pairs of a body inside its interior rectangle are settled in bulk as eligible with
        // alpha 1, exactly what the per-pair pass below would record for them.
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const float lx = fminf(w.d.c0x[b], w.d.cx[b]), ly = fminf(w.d.c0y[b], w.d.cy[b]);
          const float hx = fmaxf(w.d.c0x[b], w.d.cx[b]), hy = fmaxf(w.d.c0y[b], w.d.cy[b]);
          bool in;
          if (b == B_PK) {
            in = inside(kInteriorPuck, lx, ly, hx, hy);  // a circle's core is its centre
          } else {
            const float(&e)[4] = cb.e[b];
            const float rot = SC.rcore[b] * fabsf(w.d.a[b] - w.d.a0[b]);
            in = inside(kInteriorPlayer, lx + e[0] - rot, ly + e[1] - rot, hx + e[2] + rot, hy + e[3] + rot);
          }
          if (in && w.d.awake[b]) settled |= kEdgeMask[b];
        }
        settled &= kToiPairs & w.enabled;
        elig |= settled;
        w.toiflag |= settled;
        below &= ~settled;
        // The rest of the first pass has no order-dependent side effect either, so it runs as a uniform loop
        // over the compile-time TOI pair table (scene data as literals, per-lane predicates) instead of each
        // lane walking its own pairs through LDS lookups: the same flags and far tests, so the same queue.
        const uint32_t open = kToiPairs & w.enabled & ~settled;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (!((kToiPairs >> p) & 1u)) continue;
          const uint32_t bit = 1u << p;
          const bool live = (open & bit) && w.d.awake[SC.pbodyB[p]];
          elig |= live ? bit : 0u;
          const bool far = live && pair_far_toi(w, p, cb, SC);
          below &= far ? ~bit : ~0u;
          pending |= (live && !far) ? bit : 0u;
        }
        w.toiflag |= elig;
        todo = 0u;
      } else {
        // Later passes: an event re-enables TOI only on the moved dynamic body's contacts (their flags were
        // cleared).  Every other pair keeps its eligibility and cached alpha (cached pairs are eligible;
        // the rest were skipped for reasons no event changes), so only `redo` is visited.
        elig = w.toiflag & w.enabled & ~exhausted;
        todo = redo & kToiPairs & w.enabled & ~exhausted & ~w.toiflag;
      }
      // in pair order, per lane: eligibility, sweep alignment and the far test of the pairs still open
      while (todo) {
        const int p = __ffs(todo) - 1;
        todo &= todo - 1u;
        const uint32_t bit = 1u << p;
        const int bA = SLDS.pbodyA[p], bB = SLDS.pbodyB[p];
        if (!pick(w.d.awake, bB, 0)) continue;
        elig |= bit;
        w.toiflag |= bit;
        const float a0A = LDS(w, kLdsSal0 + bA - 3), a0B = pick(w.d.al0, bB, 0.0f);
        if (a0A < a0B) {
          LDS(w, kLdsSal0 + bA - 3) = a0B;  // static b2Sweep::Advance: only alpha0 moves
        } else if (a0B < a0A) {
          toi_drain(w, pending, below);  // keep the sequential order for this lane (see above)
          Sweep sw = body_sweep(w, bB);
          sweep_advance(sw, a0A);
          body_set_sweep(w, bB, sw);
        }
        if (pair_far_toi(w, p, cb, SLDS)) {
          below &= ~bit;
        } else {
          pending |= bit;
        }
      }
      first = false;
    }
    HK_TIC(T, 6);  // diagnostics: scan pass -> "toi-scan"
    // (2) the queued b2TimeOfImpact calls of the whole wave, dealt out over all its lanes
    toi_drain_wave(w, pending, below);
    HK_TIC(T, 7);  // diagnostics: b2TimeOfImpact -> "toi-solve" slot
    if (!act) continue;
    // (3) Box2D's minimum: first pair (in order) with the smallest alpha.  Pairs at alpha 1 never win the
    //     strict comparison, so only the lane's eligible pairs below 1 are visited (usually none or one).
    int minc = -1;
    float minAlpha = 1.0f;
    for (uint32_t m = elig & below; m; m &= m - 1u) {
      const int p = __ffs(m) - 1;
      const float alpha = LDS(w, kLdsToi + p);
      if (alpha < minAlpha) { minc = p; minAlpha = alpha; }
    }
    if (minc < 0 || 1.0f - 10.0f * kFltEps < minAlpha) {
      act = false;
      continue;
    }
    // ---- one TOI event (per-lane pair) ----
    const int bA = SLDS.pbodyA[minc], bB = SLDS.pbodyB[minc];  // static A, dynamic B
    const uint32_t mbit = 1u << minc;
    const Sweep backA = body_sweep(w, bA), backB = body_sweep(w, bB);
    body_advance(w, bA, minAlpha);
    body_advance(w, bB, minAlpha);
    pair_update_near(w, minc);  // the broad-phase shortcut only ever skips narrow phases that find no contact
    HK_TIC(T, 8);  // diagnostics: TOI event advance + contact update
    w.toiflag &= ~mbit;
    const float cnt = LDS(w, kLdsCnt + minc) + 1.0f;
    LDS(w, kLdsCnt + minc) = cnt;
    if (cnt > (float)kMaxSubSteps) exhausted |= mbit;
    if (!(w.enabled & mbit) || !(w.touch & mbit)) {
      w.enabled &= ~mbit;
      body_set_sweep(w, bA, backA);
      body_set_sweep(w, bB, backB);
      sync_xf(w, bA);
      sync_xf(w, bB);
      redo = 0u;  // sweeps restored: every other pair's flag and alpha stand
      continue;
    }
    w.n_toi++;
    set_awake(w, bA, 1);
    set_awake(w, bB, 1);
    w.bisl = (1u << bA) | (1u << bB);
    w.cisl |= mbit;
    uint32_t extra = 0u;  // other island contacts, added in B's (ascending) edge order
    int nc = 1;
    // B's contacts with static bodies (its TOI pairs) not yet in the island.  Their broad-phase tests read only
    // B's advanced pose and the scene, so they run first as a uniform loop over the compile-time pair table; a
    // rejected pair's b2Contact::Update (not touching: enabled, touching bit, wake-ups of awake bodies) changes
    // only its own bits, so it commutes with the other updates, and its tentative advance of the static body is
    // undone in the per-lane walk anyway.  The remaining (near) pairs keep the walk in edge order.
    const uint32_t cand = pick(kEdgeMask, bB, 0u) & kToiPairs & ~w.cisl;
    uint32_t m = 0u;
    {
      CoreBoxes cbe;
      core_boxes(w, cbe);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (!((kToiPairs >> p) & 1u)) continue;
        const uint32_t bit = 1u << p;
        if (!(cand & bit)) continue;
        if (pair_far_collide(w, p, &cbe, SC)) pair_update_far(w, p, SC);
        else m |= bit;
      }
    }
    while (m) {
      const int e = __ffs(m) - 1;
      m &= m - 1u;
      const uint32_t ebit = 1u << e;
      const int other = SLDS.pbodyA[e];  // the static body of a TOI pair
      const Sweep backup = body_sweep(w, other);
      if (!((w.bisl >> other) & 1u)) body_advance(w, other, minAlpha);
      pair_update_near(w, e);
      if (!(w.enabled & ebit) || !(w.touch & ebit)) {
        body_set_sweep(w, other, backup);
        continue;
      }
      w.cisl |= ebit;
      extra |= ebit;
      ++nc;
      w.bisl |= 1u << other;
    }
    HK_TIC(T, 9);  // diagnostics: TOI island build
    const float sub_dt = (1.0f - minAlpha) * dt;
    if (nc > kBigC) { w.overflow = 1; nc = kBigC; }
    // Per lane: a one-contact mini-island on register slots takes the lean routine.  In a round whose event lanes
    // all hold one (98.5 % of events on the bench workload) the wave runs the lean routine alone; in a mixed round
    // the two groups run one after the other, each lane the routine its own contacts ask for.  A wave-uniform vote
    // here (lean only if every event lane agrees) computed the same bits but made the kernel spill: 56 B of scratch
    // per lane against 16 with this form (make resource-usage; DESIGN.md, Status at r19).
    if (nc == 1 && !w.force_big) {
      toi_island_solve_one(w, minc, bA, bB, sub_dt, T);
    } else if (nc <= kToiC && !w.force_big) {
      RegSlots<kToiC> S;
      toi_island_solve(w, S, minc, extra, nc, bB, sub_dt, T);
    } else {
      w.n_big++;
      HbmSlots S{w.ws, w.n, w.a};
      toi_island_solve(w, S, minc, extra, nc, bB, sub_dt, T);
    }
    // reset island flags; invalidate the TOIs of the displaced dynamic body
    w.bisl = 0u;
    const uint32_t em = pick(kEdgeMask, bB, 0u);
    w.toiflag &= ~em;
    w.cisl &= ~em;
    redo = em;
  }
}

// b2World::Step (hockey_env.py:682)
HK_DEV void world_step(Arena &w, PhaseT &T) {
  const float dt = 0.02f;
  collide(w);
  HK_TIC(T, 1);
  HK_TRACE_POINT(w, 0);
  bool done = false;
  if (!w.force_big) {
    RegSlots<kIslandC> S;
    done = solve_islands(w, S, dt, T);
  }
  if (!done) {  // more island contacts than register slots: identical solve on the HBM slot file
    w.n_big++;
    HbmSlots S{w.ws, w.n, w.a};
    solve_islands(w, S, dt, T);
  }
  HK_TIC(T, 4);  // diagnostics: position iterations + sleep
  HK_TRACE_POINT(w, 1);
  solve_toi(w, dt, T);
  HK_TIC(T, 5);
  HK_TRACE_POINT(w, 2);
#pragma unroll
  for (int b = 0; b < 3; ++b) { w.d.fx[b] = 0.0f; w.d.fy[b] = 0.0f; w.d.tq[b] = 0.0f; }
}

}  // namespace hk

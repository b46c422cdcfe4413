// hk_velocity.h -- the 180 velocity iterations of the contact solver: the exact periodic early exit, the
// velocity-loop families and the dispatch that picks a wave's loop from what all its running lanes hold.
#pragma once
// (included from hk_solver.h, which provides FSlot, the body access, the contact rows and the slot files)
#include <type_traits>

namespace hk {

// ------------------------------------------------------------------------------------------------
// Exact early exit of the 180 velocity iterations.  One iteration is a deterministic map F of the
// solver state X = (dynamic body velocities, accumulated normal / tangent impulses).  We snapshot X at
// every iteration it = 3 (mod 4) and compare it bitwise with the snapshot from it - 4: equality means
// F^4 has a fixed point there, so X_k is 4-periodic from it - 4 on and, because 179 - it = 0 (mod 4),
// X_179 == X_it.  Stopping at `it` therefore returns exactly what 180 iterations return (periods 1, 2
// and 4 are caught).  On the oracle's strong-vs-strong workload ~99% of island solves and ~96% of TOI
// solves become periodic, most within 4-12 iterations.
// ------------------------------------------------------------------------------------------------
// Velocity-loop families and the wave's re-dispatch.  A wave runs the cheapest loop that covers the lanes
// still iterating, and re-picks it every few iterations: most solves exit periodic within 8-16 iterations,
// and the wave's 180-iteration tail then runs only the code its remaining lanes need (one-contact before
// two-contact before the general slot loop; one-point rows without the block solver; the static-body-A
// row).  Every variant computes the same float operations in the same order for the lanes it runs, and a
// lane's snapshot chain is carried across variants of a family, so the result is bit-identical to 180
// iterations of the body-file loop.  A family switch restarts the snapshot (the next comparison is skipped).
// ------------------------------------------------------------------------------------------------
HK_DEV int chunk_end(int it) {
  const int e = it + (it < 24 ? 8 : 32);
  return e < kVelIters ? e : kVelIters;
}
static_assert(kVelIters % 4 == 0, "the snapshot period divides the iteration count");
// A family's loop control: the iteration count, the running chunk's end, the first iteration whose snapshot has a
// predecessor taken by this family, and whether the lane still iterates.  The family builds it, sets `stop` for
// each chunk and hands it to the chunk by value; the chunk returns it (its own local while its loop runs).
// trip(compare): four iterations and the snapshot step; compare: a snapshot equal to its predecessor may stop the lane.
struct Chunk {
  int it, stop, first;
  bool active;
  template <typename Trip>
  HK_DEV void run(Trip &&trip) {
    for (; it < stop && active; it += 4) trip(it + 3 >= first);
    if (it >= kVelIters) active = false;  // 180 iterations done
  }
};

// One snapshot step over state words [LO, HI): compares x with the previous snapshot sn, replaces it and
// returns the OR of the differences (0: these words are where they were 4 iterations ago).
template <int LO, int HI, int N>
HK_DEV uint32_t snap_step(const uint32_t (&x)[N], uint32_t (&sn)[N]) {
  uint32_t d = 0u;
#pragma unroll
  for (int k = LO; k < HI; ++k) {
    d |= x[k] ^ sn[k];
    sn[k] = x[k];
  }
  return d;
}
// One contact's half of a snapshot, the ten words x[O .. O+9]: body B's vx, vy, w (where gB); body A's (where gA);
// ni[0], ni[1], ti[0], ti[1] (where gI).  A gated-off word is 0.  kP == 1: the second point's impulses keep the
// previous snapshot's word, so they never differ (see vone_chunk).
HK_DEV uint32_t snap_word(bool g, float f) { return g ? __float_as_uint(f) : 0u; }
template <int O, int kP = 0, int N>
HK_DEV void snap_half(uint32_t (&x)[N], const uint32_t (&sn)[N], bool gB, f2 vB, float wB, bool gA, f2 vA, float wA,
                      bool gI, const FSlot &s) {
  x[O] = snap_word(gB, vB[0]), x[O + 1] = snap_word(gB, vB[1]), x[O + 2] = snap_word(gB, wB);
  x[O + 3] = snap_word(gA, vA[0]), x[O + 4] = snap_word(gA, vA[1]), x[O + 5] = snap_word(gA, wA);
  x[O + 6] = snap_word(gI, s.ni[0]), x[O + 8] = snap_word(gI, s.ti[0]);
  x[O + 7] = kP == 1 ? sn[O + 7] : snap_word(gI, s.ni[1]), x[O + 9] = kP == 1 ? sn[O + 9] : snap_word(gI, s.ti[1]);
}
// a static body A is +0 at every solve, as get_vel_a returns it (m = lane_mask(dynamic): 0 clears the velocity to
// +0 bit for bit, without an exec branch)
HK_DEV void reset_static(f2 &v, float &w, uint32_t m) {
  v = f2{mask_f(v[0], m), mask_f(v[1], m)};
  w = mask_f(w, m);
}
// A slot's accumulated impulses, kept for a lane that only rides along in a chunk: the rider computes a dummy
// contact on that slot, which may hold another island's retired contact, and gets the impulses back afterwards.
struct SlotImpulses {
  float ni[2], ti[2];
  HK_DEV void save(const FSlot &s) {
    ni[0] = s.ni[0], ni[1] = s.ni[1], ti[0] = s.ti[0], ti[1] = s.ti[1];
  }
  HK_DEV void restore_unless(FSlot &s, bool keep) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      s.ni[j] = keep ? s.ni[j] : ni[j];
      s.ti[j] = keep ? s.ti[j] : ti[j];
    }
  }
};
// A wave-uniform vote as a template integer: fn(kint<A>) where c holds, else fn(kint<B>).  pick_points: the point
// count of a row from the votes "every running lane has one point" / "... two points" (0: mixed).
template <int K>
using kint = std::integral_constant<int, K>;
template <int A, int B, typename Fn>
HK_DEV void pick(bool c, Fn &&fn) {
  if (c) fn(kint<A>{});
  else fn(kint<B>{});
}
template <typename Fn>
HK_DEV void pick_points(bool p1, bool p2, Fn &&fn) {
  if (p1) fn(kint<1>{});
  else if (p2) fn(kint<2>{});
  else fn(kint<0>{});
}

// One-contact family (the common case, and the usual owner of a wave's 180-iteration tail): the two bodies'
// velocities stay in locals for the whole loop instead of round-tripping through the body file's selects
// every iteration.  A static body's velocity is re-read as +0 at every iteration, exactly what get_vel
// returns in the general loop; the snapshot compares the same values the general loop compares.
// kSA: no running lane has a dynamic body A, so A's velocity row is dropped (fslot_solve_velocity_p).
template <bool kSA, int kP>
HK_DEV Chunk vone_chunk(FSlot &s, bool dynA, uint32_t mA, f2 &vA, float &wA, f2 &vB, float &wB, uint32_t (&sn)[10],
                        Chunk c) {
  if constexpr (kSA && kP == 1) HK_MARK(vone_begin_s1);
  else if constexpr (kSA && kP == 2) HK_MARK(vone_begin_s2);
  else if constexpr (kSA) HK_MARK(vone_begin_s0);
  else if constexpr (kP == 1) HK_MARK(vone_begin_d1);
  else if constexpr (kP == 2) HK_MARK(vone_begin_d2);
  else HK_MARK(vone_begin_d0);
  c.run([&](bool compare) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // kSA: no running lane has a dynamic body A, and the static-A row neither reads nor writes A's velocity
      // (nor is it written back for a static body), so the reset is dead there and skipped
      if constexpr (!kSA) reset_static(vA, wA, mA);
      fslot_solve_velocity_p<kSA, kP>(s, vA, wA, vB, wB);
    }
    // kSA: every running lane's body-A words are 0; kP == 1: every running lane solves one point, so the second
    // point's impulses never change in this chunk or a later one of this family (the running set only shrinks and
    // keeps kP == 1) and are left out of the comparison
    uint32_t x[10];
    snap_half<0, kP>(x, sn, true, vB, wB, !kSA && dynA, vA, wA, true, s);
    const uint32_t diff = snap_step<0, 10>(x, sn);
    if (compare && diff == 0u) c.active = false;
  });
  HK_MARK(vone_end);
  return c;
}
HK_DEV void vone_family(FSlot &s, Dyn &B, int &it, bool &active, int first) {
  const bool entered = active;
  const int bA = fs_bA(s), bB = fs_bB(s), vc = fs_vcount(s);
  const bool dynA = bA < 3;
  const uint32_t mA = lane_mask(dynA);
  v2 vA2, vB2;
  float wA, wB;
  get_vel_a(B, bA, vA2, wA);
  get_vel_b(B, bB, vB2, wB);
  f2 vA = F2(vA2), vB = F2(vB2);
  uint32_t sn[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) sn[k] = 0u;
  Chunk c{it, it, first, active};
  while (wave_any(c.active)) {
    c.stop = chunk_end(c.it);
    const bool sa = !wave_any(c.active && dynA);
    const bool p1 = !wave_any(c.active && vc != 1), p2 = !wave_any(c.active && vc != 2);
    pick<1, 0>(sa, [&](auto kSA) {
      pick_points(p1, p2, [&](auto kP) {
        c = vone_chunk<decltype(kSA)::value != 0, decltype(kP)::value>(s, dynA, mA, vA, wA, vB, wB, sn, c);
      });
    });
  }
  it = c.it;
  active = c.active;
  if (entered) {
    if (dynA) set_vel_a(B, bA, V2(vA), wA);
    set_vel_b(B, bB, V2(vB), wB);
  }
}

// The one-contact family for callers that know body A to be static on every lane (the lean TOI event path): the
// kSA arms of vone_family alone, on body B's velocity in the caller's locals.  For such a lane vone_family picks
// the same arms (its `sa` vote holds), reads body A as +0 and never writes it, and its snapshot words of body A are 0
// either way: the same chunks, the same exit.  first == 7 as velocity_iterations starts its first family.
HK_DEV int vone_family_static_a(FSlot &s, f2 &vB, float &wB) {
  const int vc = fs_vcount(s);
  f2 vA = f2{0.0f, 0.0f};
  float wA = 0.0f;
  uint32_t sn[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) sn[k] = 0u;
  Chunk c{0, 0, 7, true};
  while (wave_any(c.active)) {
    c.stop = chunk_end(c.it);
    const bool p1 = !wave_any(c.active && vc != 1), p2 = !wave_any(c.active && vc != 2);
    pick_points(p1, p2, [&](auto kP) { c = vone_chunk<true, decltype(kP)::value>(s, false, 0u, vA, wA, vB, wB, sn, c); });
  }
  return c.it;
}

// Two-contact family (at most two live contacts; a one-contact lane runs it with contact 1 masked off).
// Each contact keeps its two bodies' velocities in locals; after a contact is solved, the other contact's
// copy of any body it shares (equal body index) is refreshed from it, so every solve reads exactly the
// velocities the body-file loop reads, at 2 selects per shared-body component instead of the body file's
// gather and scatter.  A static body A is +0 at every solve, as get_vel_a returns it.  The snapshot covers
// every island body (each appears in some contact) and both contacts' impulses: the set the general loop
// compares, some bodies twice.  When the two contacts belong to different islands (`sep`: no shared
// dynamic body), each contact's half of the snapshot is its island's whole state, so a contact whose half
// is periodic retires on its own (on0 / on1 false) while the other keeps iterating (see velocity_iterations).
HK_DEV f2 sel2(bool c, f2 a, f2 b) { return f2{c ? a[0] : b[0], c ? a[1] : b[1]}; }
struct TwoState {
  f2 vA0, vB0, vA1, vB1;
  float wA0, wB0, wA1, wB1;
};
// What a two-contact lane holds for one family entry (built once by vtwo_family, read-only in the chunks): contact
// 1 is live; the contacts are two islands; the lane's shape (s2_shape, tb_shape); contact 0's / 1's body A is
// dynamic, and their lane masks (reset_static); contact 1's body A / B is contact 0's body A / B.
struct TwoLane {
  bool two, sep, s2, tb, dA0, dA1;
  uint32_t mA0, mA1;
  bool a1a0, a1b0, b1a0, b1b0;
};
// kG: some lane has retired contact 0 (it is then skipped by a per-lane branch; otherwise solved unguarded)
template <int kP0, int kP1, bool kG>
HK_DEV Chunk vtwo_chunk(FSlot &s0, FSlot &s1, TwoState &t, uint32_t (&sn)[20], const TwoLane L, Chunk c, bool &on0,
                        bool &on1) {
  // the state lives in this function's own locals for the loop (selects between fields of a by-reference
  // struct turn into pointer selects, which keep the struct in scratch memory)
  f2 vA0 = t.vA0, vB0 = t.vB0, vA1 = t.vA1, vB1 = t.vB1;
  float wA0 = t.wA0, wB0 = t.wB0, wA1 = t.wA1, wB1 = t.wB1;
  HK_MARK(vtwo_begin);
  c.run([&](bool compare) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!kG || on0) {
        reset_static(vA0, wA0, L.mA0);
        fslot_solve_velocity_p<false, kP0>(s0, vA0, wA0, vB0, wB0);
        vA1 = sel2(L.a1a0, vA0, sel2(L.a1b0, vB0, vA1));
        wA1 = L.a1a0 ? wA0 : (L.a1b0 ? wB0 : wA1);
        vB1 = sel2(L.b1a0, vA0, sel2(L.b1b0, vB0, vB1));
        wB1 = L.b1a0 ? wA0 : (L.b1b0 ? wB0 : wB1);
      }
      if (on1) {
        reset_static(vA1, wA1, L.mA1);
        fslot_solve_velocity_p<false, kP1>(s1, vA1, wA1, vB1, wB1);
        vA0 = sel2(L.a1a0, vA1, sel2(L.b1a0, vB1, vA0));
        wA0 = L.a1a0 ? wA1 : (L.b1a0 ? wB1 : wA0);
        vB0 = sel2(L.a1b0, vA1, sel2(L.b1b0, vB1, vB0));
        wB0 = L.a1b0 ? wA1 : (L.b1b0 ? wB1 : wB0);
      }
    }
    uint32_t x[20];
    snap_half<0>(x, sn, true, vB0, wB0, L.dA0, vA0, wA0, true, s0);
    snap_half<10>(x, sn, L.two, vB1, wB1, L.dA1, vA1, wA1, L.two, s1);
    const uint32_t d0 = snap_step<0, 10>(x, sn), d1 = snap_step<10, 20>(x, sn);
    if (compare) {
      if (L.sep) {
        on0 = on0 && d0 != 0u;
        on1 = on1 && d1 != 0u;
        if (on0 != on1) HK_HOST_DIAG_INC(0);
      } else if ((d0 | d1) == 0u) {
        on0 = false;
        on1 = false;
      }
      if (!on0 && !on1) c.active = false;
    }
  });
  HK_MARK(vtwo_end);
  t.vA0 = vA0; t.vB0 = vB0; t.vA1 = vA1; t.vB1 = vB1;
  t.wA0 = wA0; t.wB0 = wB0; t.wA1 = wA1; t.wB1 = wB1;
  return c;
}
// The tail's two-contact shape (scripts/tail_shape_study.c: ~90 % of the two-contact family's iterations from
// iteration 56 on): one island whose contact 1 has a static body A and contact 0's body A as its body B (b1 == a0:
// player-puck, then wall-player), optionally with one-contact lanes riding along.  The shared body has ONE home
// (contact 0's A locals): contact 1 reads it directly and its update is committed back with one select per component
// (riders discard theirs), instead of the generic chunk's per-lane refresh selects after both contacts and its
// exec-mask guard on contact 1; contact 1 runs the static-body-A row.  Riders (two == false) compute a dummy contact
// 1 on their own slot 1, whose impulses are restored at the chunk's end (that slot may hold another island's retired
// contact); their snapshot words of contact 1 are 0, as in the generic chunk.  Every S2 lane's float operations are
// the generic chunk's, in its order, so the result is bit-identical; the snapshot words keep their meaning (contact
// 1's body B words are the shared body's, contact 1's static body A words are 0), so the chain carries across.
template <int kP0, int kP1>
HK_DEV Chunk vtwo_s2_chunk(FSlot &s0, FSlot &s1, TwoState &t, uint32_t (&sn)[20], const TwoLane L, Chunk c, bool &on0,
                           bool &on1) {
  f2 vA0 = t.vA0, vB0 = t.vB0;
  float wA0 = t.wA0, wB0 = t.wB0;
  if (c.active && L.two) HK_HOST_DIAG_INC(3);
  SlotImpulses rider;
  rider.save(s1);
  HK_MARK(vtwo_s2_begin);
  c.run([&](bool compare) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      reset_static(vA0, wA0, L.mA0);  // a rider's static A
      fslot_solve_velocity_p<false, kP0>(s0, vA0, wA0, vB0, wB0);
      f2 vA1 = f2{0.0f, 0.0f}, vB1 = vA0;
      float wA1 = 0.0f, wB1 = wA0;
      fslot_solve_velocity_p<true, kP1>(s1, vA1, wA1, vB1, wB1);
      vA0 = sel2(L.two, vB1, vA0);
      wA0 = L.two ? wB1 : wA0;
    }
    uint32_t x[20];
    snap_half<0>(x, sn, true, vB0, wB0, L.dA0, vA0, wA0, true, s0);
    snap_half<10>(x, sn, L.two, vA0, wA0, false, vA0, wA0, L.two, s1);  // the shared body; static body A: 0
    const uint32_t d = snap_step<0, 20>(x, sn);
    // no lane here is split over two islands (see the dispatch)
    if (compare && d == 0u) on0 = on1 = c.active = false;
  });
  HK_MARK(vtwo_s2_end);
  t.vA0 = vA0; t.vB0 = vB0; t.wA0 = wA0; t.wB0 = wB0;
  // the generic chunks' copy of the shared body, for S2 lanes only: a lane of another shape that finished in an
  // earlier chunk runs this code too (exec is not masked here) and its copies must stay as they are
  t.vB1 = sel2(L.s2, vA0, t.vB1);
  t.wB1 = L.s2 ? wA0 : t.wB1;
  rider.restore_unless(s1, L.two);
  return c;
}

// The aliased two-contact chunk for mixed waves: every running lane is an S2 lane (b1 == a0, contact 1 static
// A), a "TB" lane (b1 == b0: contact 1's body B is contact 0's body B, e.g. wall-puck then player-puck, or a TOI
// mini-island's two static contacts on one body), or a one-contact rider -- with any point counts (scripts/
// tail_shape_study.c: the slowest waves mostly mix S2 lanes whose contact 1 has one and two points, or run TB
// lanes).  The shared body has one home per lane (contact 0's A for S2, its B for TB): contact 1 reads it through one
// select per component and commits its update with one per component and shape, instead of the generic chunk's
// refresh selects after both contacts and its exec-mask guard; contact 1's own body A lives in locals (static for
// S2, +0 by its lane mask).  Riders as in vtwo_s2_chunk.  Bit-identical to the generic chunk for every lane.
template <int kP0, int kP1>
HK_DEV Chunk vtwo_alias_chunk(FSlot &s0, FSlot &s1, TwoState &t, uint32_t (&sn)[20], const TwoLane L, Chunk c,
                              bool &on0, bool &on1) {
  f2 vA0 = t.vA0, vB0 = t.vB0, vA1 = t.vA1;
  float wA0 = t.wA0, wB0 = t.wB0, wA1 = t.wA1;
  if (c.active && L.two) HK_HOST_DIAG_INC(3);
  SlotImpulses rider;
  rider.save(s1);
  HK_MARK(vtwo_alias_begin);
  c.run([&](bool compare) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      reset_static(vA0, wA0, L.mA0);
      fslot_solve_velocity_p<false, kP0>(s0, vA0, wA0, vB0, wB0);
      f2 vB1 = sel2(L.s2, vA0, vB0);  // the shared body (a rider: a dummy copy)
      float wB1 = L.s2 ? wA0 : wB0;
      reset_static(vA1, wA1, L.mA1);
      fslot_solve_velocity_p<false, kP1>(s1, vA1, wA1, vB1, wB1);
      vA0 = sel2(L.s2, vB1, vA0);
      wA0 = L.s2 ? wB1 : wA0;
      vB0 = sel2(L.tb, vB1, vB0);
      wB0 = L.tb ? wB1 : wB0;
    }
    const f2 sh = sel2(L.s2, vA0, vB0);
    const float wsh = L.s2 ? wA0 : wB0;
    uint32_t x[20];
    snap_half<0>(x, sn, true, vB0, wB0, L.dA0, vA0, wA0, true, s0);
    snap_half<10>(x, sn, L.two, sh, wsh, L.dA1, vA1, wA1, L.two, s1);
    const uint32_t d = snap_step<0, 20>(x, sn);
    // no lane here is split over two islands (see the dispatch)
    if (compare && d == 0u) on0 = on1 = c.active = false;
  });
  HK_MARK(vtwo_alias_end);
  // only S2 and TB lanes' contact-1 copies changed (others ran no iteration here or are riders)
  const bool shaped = L.s2 || L.tb;
  t.vA0 = vA0; t.vB0 = vB0; t.wA0 = wA0; t.wB0 = wB0;
  t.vB1 = sel2(shaped, sel2(L.s2, vA0, vB0), t.vB1);
  t.wB1 = shaped ? (L.s2 ? wA0 : wB0) : t.wB1;
  t.vA1 = sel2(L.tb, vA1, t.vA1);
  t.wA1 = L.tb ? wA1 : t.wA1;
  rider.restore_unless(s1, L.two);
  return c;
}

// The lane shapes the specialised loops are written for, from two (three) live contacts' slot bits, in slot order:
//   S2: one island, contact 1's body A static and its body B contact 0's body A (player-puck, wall-player);
//   TB: one island, contact 1's body B is contact 0's body B;
//   S3: slot 0 = (static, X), slot 1 = (Y, X), slot 2 = (static, Y), one point each (see vthree_s3_chunk).
HK_DEV bool s2_shape(int bits0, int bits1) {
  const int a0 = (bits0 >> 7) & 15, a1 = (bits1 >> 7) & 15, b1 = (bits1 >> 11) & 15;
  return a1 >= 3 && b1 == a0 && ((bits0 >> 5) & 3) == ((bits1 >> 5) & 3);
}
HK_DEV bool tb_shape(int bits0, int bits1) {
  return ((bits1 >> 11) & 15) == ((bits0 >> 11) & 15) && ((bits0 >> 5) & 3) == ((bits1 >> 5) & 3);
}
HK_DEV bool s3_shape(const FSlot &s0, const FSlot &s1, const FSlot &s2) {
  return fs_bA(s0) >= 3 && fs_bA(s2) >= 3 && fs_bA(s1) < 3 && fs_bB(s0) == fs_bB(s1) && fs_bA(s1) == fs_bB(s2) &&
         fs_vcount(s0) == 1 && fs_vcount(s1) == 1 && fs_vcount(s2) == 1;
}

// runs until every lane is done or no running lane has both contacts live (then the one-contact family takes
// over).  on0 / on1 in: the lane's contacts that iterate (on1 == two); out: the ones still unfinished.
HK_DEV void vtwo_family(FSlot &s0, FSlot &s1, Dyn &B, bool two, int &it, bool &active, int first, bool &on0,
                        bool &on1) {
  const bool entered = active;
  const int a0 = fs_bA(s0), b0 = fs_bB(s0);
  const int a1 = two ? fs_bA(s1) : 15, b1 = two ? fs_bB(s1) : 15;  // 15: matches no body
  const int vc0 = fs_vcount(s0), vc1 = two ? fs_vcount(s1) : 1;
  const bool s2 = two && s2_shape(s0.bits, s1.bits), tb = two && tb_shape(s0.bits, s1.bits);
  const bool dA0 = a0 < 3, dA1 = a1 < 3;
  const TwoLane L{two, two && fs_isl(s0) != fs_isl(s1), s2, tb, dA0, dA1, lane_mask(dA0), lane_mask(dA1),
                  a1 == a0, a1 == b0, b1 == a0, b1 == b0};
  TwoState t;
  v2 q;
  get_vel_a(B, a0, q, t.wA0);
  t.vA0 = F2(q);
  get_vel_b(B, b0, q, t.wB0);
  t.vB0 = F2(q);
  get_vel_a(B, a1, q, t.wA1);
  t.vA1 = F2(q);
  get_vel_b(B, b1, q, t.wB1);
  t.vB1 = F2(q);
  uint32_t sn[20];
#pragma unroll
  for (int k = 0; k < 20; ++k) sn[k] = 0u;
  Chunk c{it, it, first, active};
  const auto s2_chunk = [&](auto kP0, auto kP1) {
    c = vtwo_s2_chunk<decltype(kP0)::value, decltype(kP1)::value>(s0, s1, t, sn, L, c, on0, on1);
  };
  const auto generic = [&](auto kP0, auto kP1, auto kG) {
    c = vtwo_chunk<decltype(kP0)::value, decltype(kP1)::value, decltype(kG)::value != 0>(s0, s1, t, sn, L, c, on0, on1);
  };
  while (wave_any(c.active) && wave_any(c.active && on0 && on1)) {
    c.stop = chunk_end(c.it);
    // S2 chunk: every running lane is an S2 lane with both contacts live, or a one-contact rider (two == false)
    const bool s2ok = !wave_any(c.active && (!on0 || (two && !(s2 && on1))));
    if (s2ok && !wave_any(c.active && two && vc1 != 1)) {
      pick<1, 0>(!wave_any(c.active && vc0 != 1), [&](auto kP0) { s2_chunk(kP0, kint<1>{}); });
    } else if (s2ok && !wave_any(c.active && two && vc1 != 2)) {
      pick<1, 0>(!wave_any(c.active && vc0 != 1), [&](auto kP0) { s2_chunk(kP0, kint<2>{}); });
    } else if (!wave_any(c.active && (!on0 || (two && !((s2 || tb) && on1))))) {
      // aliased chunk: S2 and TB lanes with both contacts live, and one-contact riders
      const bool p0 = !wave_any(c.active && vc0 != 1), p1 = !wave_any(c.active && two && vc1 != 1);
      pick<1, 0>(p0, [&](auto kP0) {
        pick<1, 0>(p1, [&](auto kP1) {
          c = vtwo_alias_chunk<decltype(kP0)::value, decltype(kP1)::value>(s0, s1, t, sn, L, c, on0, on1);
        });
      });
    } else if (wave_any(c.active && !on0))
      generic(kint<0>{}, kint<0>{}, kint<1>{});
    else if (!wave_any(c.active && (vc0 != 1 || vc1 != 1)))
      generic(kint<1>{}, kint<1>{}, kint<0>{});
    // a wave whose running lanes agree on both point counts runs the rows without the other count's code (a
    // lane of a one-contact island rides along with contact 1 masked off, whatever kP1 says)
    else if (!wave_any(c.active && (vc0 != 1 || (two && vc1 != 2))))
      generic(kint<1>{}, kint<2>{}, kint<0>{});
    else if (!wave_any(c.active && (vc0 != 2 || (two && vc1 != 1))))
      generic(kint<2>{}, kint<1>{}, kint<0>{});
    else if (!wave_any(c.active && (vc0 != 2 || (two && vc1 != 2))))
      generic(kint<2>{}, kint<2>{}, kint<0>{});
    else
      generic(kint<0>{}, kint<0>{}, kint<0>{});
  }
  it = c.it;
  active = c.active;
  if (entered) {
    if (dA0) set_vel_a(B, a0, V2(t.vA0), t.wA0);
    set_vel_b(B, b0, V2(t.vB0), t.wB0);
    if (two) {
      if (dA1) set_vel_a(B, a1, V2(t.vA1), t.wA1);
      set_vel_b(B, b1, V2(t.vB1), t.wB1);
    }
  }
}

// The tail's three-contact shape (scripts/tail_shape_study.c): one island of three one-point contacts, slot 0
// = (static, X), slot 1 = (Y, X), slot 2 = (static, Y) -- wall-puck, player-puck, wall-player -- optionally with
// riders: one-contact lanes (their contact swapped into slot 0) and S2 two-contact lanes (player-puck, wall-player:
// their live contacts swapped into slots 0 and 1, as the two-contact family holds them; the slowest waves of the
// bench workload mostly hold S3 and S2 lanes together).  X and Y live in locals, aliased at compile time, instead of
// the general family's body-file gathers and scatters (~30 selects per contact): slot 0 runs the generic row on
// (A0, X) (a rider's own bodies; an S3 lane's A0 is static, +0), slot 1 the dynamic row on (Y, X) -- an S2 lane's
// on (+0, A0), its static body A and its body B, contact 0's body A, by one select per component in and out (the
// row with a +0 body A is bit-identical to the static-body-A row: see fslot_solve_velocity_p) -- whose update of X a
// non-S3 lane discards, slot 2 the static-body-A row on Y, S3 lanes only in effect.  Non-S3 lanes' slot 2
// impulses, and one-contact riders' slot 1 impulses, are restored at the end (another island's retired contacts may
// sit there).  The snapshot covers X, Y, A0 and the impulses of the slots the lane solves: the island's whole
// state, so the periodic exit stays exact; this family starts its own chain.  Each lane's float operations are the
// general / two-contact families', in their order.  Runs while some S3 lane iterates.
template <int kP0, int kP1>
HK_DEV Chunk vthree_s3_chunk(FSlot &s0, FSlot &s1, FSlot &s2, bool s3, bool s2l, uint32_t mA0, uint32_t mY, bool dA0,
                             f2 &vA0, float &wA0, f2 &vX, float &wX, f2 &vY, float &wY, uint32_t (&sn)[19], Chunk c) {
  HK_MARK(vthree_begin);
  c.run([&](bool compare) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      reset_static(vA0, wA0, mA0);  // static A: every S3 lane, static riders
      fslot_solve_velocity_p<false, kP0>(s0, vA0, wA0, vX, wX);
      f2 vB1 = sel2(s2l, vA0, vX);  // an S2 lane's contact 1 acts on its body A0
      float wB1 = s2l ? wA0 : wX;
      reset_static(vY, wY, mY);  // an S2 lane's contact 1 has a static body A
      fslot_solve_velocity_p<false, kP1>(s1, vY, wY, vB1, wB1);
      vX = sel2(s3, vB1, vX);
      wX = s3 ? wB1 : wX;
      vA0 = sel2(s2l, vB1, vA0);
      wA0 = s2l ? wB1 : wA0;
      f2 vA2 = f2{0.0f, 0.0f};
      float wA2 = 0.0f;
      fslot_solve_velocity_p<true, 1>(s2, vA2, wA2, vY, wY);
    }
    const bool sl1 = s3 || s2l;  // lanes that solve slot 1
    uint32_t x[19];
    snap_half<0>(x, sn, true, vX, wX, dA0, vA0, wA0, true, s0);
    x[10] = snap_word(s3, vY[0]), x[11] = snap_word(s3, vY[1]), x[12] = snap_word(s3, wY);
    x[13] = snap_word(sl1, s1.ni[0]), x[14] = snap_word(sl1, s1.ti[0]);
    x[15] = snap_word(sl1, s1.ni[1]), x[16] = snap_word(sl1, s1.ti[1]);
    x[17] = snap_word(s3, s2.ni[0]), x[18] = snap_word(s3, s2.ti[0]);
    const uint32_t d = snap_step<0, 19>(x, sn);
    if (compare && d == 0u) c.active = false;
  });
  HK_MARK(vthree_end);
  return c;
}
// s3: an S3 lane; s2l: an S2 lane (its contacts in slots 0 and 1); else a one-contact rider (slot 0)
HK_DEV void vthree_s3_family(FSlot &s0, FSlot &s1, FSlot &s2, Dyn &B, bool s3, bool s2l, int &it, bool &active,
                             int first) {
  const bool entered = active;
  const int a0 = fs_bA(s0), x = fs_bB(s0), y = s3 ? fs_bA(s1) : x;
  const bool dA0 = a0 < 3;
  const uint32_t mA0 = lane_mask(dA0), mY = lane_mask(s3);
  v2 q;
  float wA0, wX, wY;
  get_vel_a(B, a0, q, wA0);
  f2 vA0 = F2(q);
  get_vel_b(B, x, q, wX);
  f2 vX = F2(q);
  get_vel_b(B, y, q, wY);
  f2 vY = F2(q);
  SlotImpulses rider1, rider2;
  rider1.save(s1);
  rider2.save(s2);
  uint32_t sn[19];
#pragma unroll
  for (int k = 0; k < 19; ++k) sn[k] = 0u;
  // the point-count variant is picked once per family entry (the running set only shrinks, so one-point stays
  // one-point), and each variant gets a loop of its own (the lambda is instantiated once per variant): picking it
  // per chunk inside one loop made the kernel spill (both variants' invariants hoisted together; 16 -> 152 B of
  // scratch per lane, make resource-usage)
  Chunk c{it, it, first, active};
  pick<1, 0>(!wave_any(active && (fs_vcount(s0) != 1 || (s2l && fs_vcount(s1) != 1))), [&](auto kP) {
    while (wave_any(c.active && s3)) {
      c.stop = chunk_end(c.it);
      c = vthree_s3_chunk<decltype(kP)::value, decltype(kP)::value>(s0, s1, s2, s3, s2l, mA0, mY, dA0, vA0, wA0, vX, wX,
                                                                    vY, wY, sn, c);
    }
  });
  it = c.it;
  active = c.active;
  if (entered) {
    if (dA0) set_vel_a(B, a0, V2(vA0), wA0);
    set_vel_b(B, x, V2(vX), wX);
    if (s3) set_vel_b(B, y, V2(vY), wY);
  }
  rider1.restore_unless(s1, s3 || s2l);
  rider2.restore_unless(s2, s3);
}

// General family: the slot loop over the body file (any island size, register or HBM slots).  Islands
// share no dynamic body, so each island's state (its bodies' velocities, its contacts' impulses) evolves
// on its own: an island whose state is periodic retires on its own (its slots leave `live` and are no
// longer solved; its state at iteration 179 is the current one), while the lane's other islands keep
// iterating.  With `leave`, it returns after a chunk once no running lane has more than two live contacts.
// kP == 1: every live contact of every running lane has one point (the caller checks at entry; the running set and
// the live contacts only shrink), so the rows skip the block solver and the per-slot point-count branch.
template <typename SL, int kP = 0>
HK_DEV void vgen_family(SL &S, Dyn &B, int nc, uint32_t &live, const int (&isl_of)[3], int &it, bool &active,
                        int first, bool leave) {
  uint32_t sb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) sb[k] = 0u;
  uint32_t im0 = 0u, im1 = 0u, im2 = 0u;  // slots of islands 0, 1, 2
  S.each(nc, [&](FSlot &s, int i) {
    s.sn[0] = s.sn[1] = s.sn[2] = s.sn[3] = 0u;
    const int k = fs_isl(s);
    im0 |= k == 0 ? 1u << i : 0u;
    im1 |= k == 1 ? 1u << i : 0u;
    im2 |= k == 2 ? 1u << i : 0u;
  });
  Chunk c{it, it, first, active};
  while (wave_any(c.active)) {
    if (leave && !wave_any(c.active && __popc(live) > 2)) break;
    c.stop = chunk_end(c.it);
    HK_MARK(vit_begin);
    c.run([&](bool compare) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        S.each(nc, [&](FSlot &s, int i) {
          if ((live >> i) & 1u) fslot_solve_velocity<kP>(s, B);
        });
      uint32_t d0 = 0u, d1 = 0u, d2 = 0u;  // per-island snapshot differences
      const uint32_t xb[9] = {__float_as_uint(B.vx[0]), __float_as_uint(B.vy[0]), __float_as_uint(B.w[0]),
                              __float_as_uint(B.vx[1]), __float_as_uint(B.vy[1]), __float_as_uint(B.w[1]),
                              __float_as_uint(B.vx[2]), __float_as_uint(B.vy[2]), __float_as_uint(B.w[2])};
      const uint32_t db[3] = {snap_step<0, 3>(xb, sb), snap_step<3, 6>(xb, sb), snap_step<6, 9>(xb, sb)};
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        d0 |= isl_of[b] == 0 ? db[b] : 0u;
        d1 |= isl_of[b] == 1 ? db[b] : 0u;
        d2 |= isl_of[b] == 2 ? db[b] : 0u;
      }
      S.each(nc, [&](FSlot &s, int) {
        const uint32_t xs[4] = {__float_as_uint(s.ni[0]), __float_as_uint(s.ni[1]), __float_as_uint(s.ti[0]),
                                __float_as_uint(s.ti[1])};
        const uint32_t d = snap_step<0, 4>(xs, s.sn);
        const int k = fs_isl(s);
        d0 |= k == 0 ? d : 0u;
        d1 |= k == 1 ? d : 0u;
        d2 |= k == 2 ? d : 0u;
      });
      if (compare) {
        const uint32_t before = live;
        live &= (d0 == 0u ? ~im0 : ~0u) & (d1 == 0u ? ~im1 : ~0u) & (d2 == 0u ? ~im2 : ~0u);
        if (live == 0u) c.active = false;
        else if (live != before) HK_HOST_DIAG_INC(0);
      }
    });
    HK_MARK(vit_end);
  }
  it = c.it;
  active = c.active;
}

// A lane's live contacts into slots 0 and 1 for the one-, two- and three-contact families (kIn), and back: slot 0's
// partner is k0, slot 1's is k1 (per lane; k == the slot itself: no move), each exchanged where its wave-uniform
// flag says some lane moves.  In: slot order; out: the reverse, so an island's contacts keep their Gauss-Seidel
// order while the family runs and every slot is back in place afterwards.
template <bool kIn, typename SL>
HK_DEV void swap_live(SL &S, bool w0, int k0, bool w1, int k1) {
  if (kIn && w0) slot_swap(S, 0, k0);
  if (w1) slot_swap(S, 1, k1);
  if (!kIn && w0) slot_swap(S, 0, k0);
}

// 180 velocity iterations over nc slots, with the exact periodic early exit.  Register slots: the wave walks
// the families general -> two -> one as the lanes' LIVE contacts allow (contacts of islands that have not
// yet become periodic; islands retire one by one, see vgen_family / vtwo_family).  The one- and two-contact
// families run on slots 0 and 1: a lane whose live contacts sit elsewhere has them swapped there (in slot
// order, so an island's Gauss-Seidel order is kept) and back afterwards.  HBM slots: the general loop.
// isl_of[b]: island of dynamic body b (-1: none).
template <typename SL>
HK_DEV int velocity_iterations(SL &S, Dyn &B, int nc, const int (&isl_of)[3], PhaseT &T) {
  int it = 0;
  uint32_t live = nc > 0 ? (1u << nc) - 1u : 0u;
  bool active = nc > 0;
  int first = 7;  // the first comparison against a snapshot taken by this loop (it + 3 == 7)
  if constexpr (SL::kRegister) {
    static_assert(SlotCap<SL>::value >= 2, "the one- and two-contact families use slots 0 and 1");
    while (wave_any(active)) {
      const int nl = __popc(live);
      HK_FAM_T0();
      // the lane's first and second live slot (0 and 1 where it has none)
      const int j0 = nl >= 1 ? __ffs(live) - 1 : 0;
      const int j1 = nl >= 2 ? __ffs(live & (live - 1u)) - 1 : 1;
      // S3 family (vthree_s3_family): every running lane is an S3 lane (its three live contacts in slots 0-2), an
      // S2 lane (two live contacts) or a one-contact rider
      bool s3 = false, s2l = false, s3ok = false;
      if constexpr (SlotCap<SL>::value >= 3) {
        s3 = active && nl == 3 && live == 7u && s3_shape(S.s[0], S.s[1], S.s[2]);
        if (wave_any(s3)) {
          int b0 = 0, b1 = 0;  // the live slots' bits, by select (slot indices are runtime per lane)
#pragma unroll
          for (int q = 0; q < SlotCap<SL>::value; ++q) {
            b0 = q == j0 ? S.s[q].bits : b0;
            b1 = q == j1 ? S.s[q].bits : b1;
          }
          s2l = active && nl == 2 && s2_shape(b0, b1);
        }
        s3ok = wave_any(s3) && !wave_any(active && !s3 && !s2l && nl != 1);
      }
      if (s3ok) {
        if constexpr (SlotCap<SL>::value >= 3) {
          // riders' and S2 lanes' live contacts to slots 0 (and 1), in slot order, as the two-contact family has them
          const bool mv0 = !s3 && j0 != 0, mv1 = s2l && j1 != 1;
          const bool any0 = wave_any(active && mv0), any1 = wave_any(mv1);
          swap_live<true>(S, any0, mv0 ? j0 : 0, any1, mv1 ? j1 : 1);
          const bool entered = active;
          if (s3) HK_HOST_DIAG_INC(2);
          vthree_s3_family(S.s[0], S.s[1], S.s[2], B, s3, s2l, it, active, first);
          live = entered && !active ? 0u : live;
          swap_live<false>(S, any0, mv0 ? j0 : 0, any1, mv1 ? j1 : 1);
          HK_FAM_ADD(T, 0);
        }
      } else if (wave_any(active && nl > 2)) {
        bool p1 = true;  // every live contact one-point
        S.each(nc, [&](FSlot &s, int i) { p1 = p1 && (((live >> i) & 1u) == 0u || fs_vcount(s) == 1); });
        pick<1, 0>(!wave_any(active && !p1), [&](auto kP) {
          vgen_family<SL, decltype(kP)::value>(S, B, nc, live, isl_of, it, active, first, true);
        });
        HK_FAM_ADD(T, 0);
      } else {
        const bool fam2 = wave_any(active && nl > 1);
        const bool perm = wave_any(active && (j0 != 0 || (fam2 && j1 != 1)));
        if (perm && active && (j0 != 0 || (fam2 && j1 != 1))) HK_HOST_DIAG_INC(1);
        swap_live<true>(S, perm, j0, perm && fam2, j1);
        if (fam2) {
          bool on0 = active, on1 = active && nl > 1;
          vtwo_family(S.s[0], S.s[1], B, nl > 1, it, active, first, on0, on1);
          live &= (on0 ? ~0u : ~(1u << j0)) & (nl > 1 && !on1 ? ~(1u << j1) : ~0u);
          HK_FAM_ADD(T, 1);
        } else {
          const bool entered = active;
          vone_family(S.s[0], B, it, active, first);
          live = entered ? 0u : live;
          HK_FAM_ADD(T, 2);
        }
        swap_live<false>(S, perm, j0, perm && fam2, j1);
      }
      active = live != 0u && it < kVelIters;
      first = it + 7;  // the next family starts a fresh snapshot
    }
  } else {
    vgen_family(S, B, nc, live, isl_of, it, active, first, false);
  }
  return it;
}

}  // namespace hk

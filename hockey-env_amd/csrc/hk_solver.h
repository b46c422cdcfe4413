// hk_solver.h -- register-resident contact solver (the hot loop of b2Island::Solve / SolveTOI).
//
// One lane runs one arena's Gauss-Seidel loop (180 velocity iterations x island contacts, up to 60 / 20
// position iterations; Box2D 2.3 b2ContactSolver, restated by the CPU test oracle).  The island's contacts
// live in MAXS fixed register slots (loops fully unrolled, slot indices compile-time); body positions and
// velocities are the arena's register body file (Dyn), addressed by body id through select chains -- a
// static body reads as zero velocity at its fixed origin, exactly what Box2D's island arrays hold for it.
// Float operation order is the oracle's.  This file holds the slots, the contact rows and the slot files; the 180
// velocity iterations over them (loop families, wave dispatch, exact periodic exit) are hk_velocity.h.
#pragma once
// (included from hk_world.h after hk_body.h, which provides Arena / Dyn / pick / place / MF and the SC alias)

namespace hk {

// Host harness only (hostcheck, HK_HOST_DIAG): how often the velocity loop's island retirement and slot swaps
// ran, so a CPU test can show that its lockstep runs exercised them.  [0] an island retired while another
// of its lane's islands kept iterating, [1] a lane's live contacts were swapped into slots 0/1, [2] an S3 lane
// entered the three-contact shape family, [3] an S2 lane ran a two-contact shape chunk.
#ifdef HK_HOST_DIAG
extern unsigned long long g_hk_host_diag[4];
#define HK_HOST_DIAG_INC(k) (++g_hk_host_diag[k])
// TOI events that took the lean one-contact path (hk_world.h toi_island_solve_one); a counter of its own, so the
// four above keep their indices and hkh_diag its size
extern unsigned long long g_hk_host_toi_lean;
#define HK_HOST_TOI_LEAN_INC() (++g_hk_host_toi_lean)
#else
#define HK_HOST_DIAG_INC(k) ((void)0)
#define HK_HOST_TOI_LEAN_INC() ((void)0)
#endif


// One contact of the solver.  Only what the velocity iterations touch lives here (36 words); the
// position-phase geometry (manifold points / normal, local centres, radii, static origins) is re-read from
// the in-place HBM manifold and the scene when a position pass or InitializeVelocityConstraints needs it,
// so it is not live in registers across the 180-iteration velocity loop.
struct FSlot {
  int bits;  // pair | island << 5 | bodyA << 7 | bodyB << 11 | vcount << 15 | pcount << 17 | type << 19
  float mA, mB, iA, iB, fr;
  float nx, ny;
  float rAx[2], rAy[2], rBx[2], rBy[2], ni[2], ti[2], nm[2], tm[2], bias[2];
  float Kxx, Kxy, Kyy, Nxx, Nxy, Nyy;  // K and its inverse are symmetric (Box2D stores ex.y == ey.x)
  uint32_t sn[4];                       // impulse snapshot for the periodic early exit (velocity_iterations)
};
constexpr int kSlotWords = (int)(sizeof(FSlot) / 4);

HK_DEV int fs_pair(const FSlot &s) { return s.bits & 31; }
HK_DEV int fs_isl(const FSlot &s) { return (s.bits >> 5) & 3; }
HK_DEV int fs_bA(const FSlot &s) { return (s.bits >> 7) & 15; }
HK_DEV int fs_bB(const FSlot &s) { return (s.bits >> 11) & 15; }
HK_DEV int fs_vcount(const FSlot &s) { return (s.bits >> 15) & 3; }
HK_DEV int fs_pcount(const FSlot &s) { return (s.bits >> 17) & 3; }
HK_DEV int fs_type(const FSlot &s) { return (s.bits >> 19) & 3; }

// body access by pair side (pick_a / pick_b / place_a: body A is never the puck, body B is dynamic)
HK_DEV void get_vel_a(const Dyn &B, int b, v2 &v, float &w) {
  v = V(pick_a(B.vx, b, 0.0f), pick_a(B.vy, b, 0.0f));
  w = pick_a(B.w, b, 0.0f);
}
HK_DEV void get_vel_b(const Dyn &B, int b, v2 &v, float &w) {
  v = V(pick_b(B.vx, b), pick_b(B.vy, b));
  w = pick_b(B.w, b);
}
HK_DEV void set_vel_a(Dyn &B, int b, v2 v, float w) {
  place_a(B.vx, b, v.x);
  place_a(B.vy, b, v.y);
  place_a(B.w, b, w);
}
HK_DEV void set_vel_b(Dyn &B, int b, v2 v, float w) {
  place(B.vx, b, v.x);
  place(B.vy, b, v.y);
  place(B.w, b, w);
}
// position of body b (a static body sits at its origin with angle 0)
HK_DEV void get_pos_a(const Dyn &B, int b, v2 &c, float &a) {
  if (b < 3) {
    c = V(pick_a(B.cx, b, 0.0f), pick_a(B.cy, b, 0.0f));
    a = pick_a(B.a, b, 0.0f);
  } else {
    c = V(SLDS.spx[b], SLDS.spy[b]);
    a = 0.0f;
  }
}
HK_DEV void get_pos_b(const Dyn &B, int b, v2 &c, float &a) {
  c = V(pick_b(B.cx, b), pick_b(B.cy, b));
  a = pick_b(B.a, b);
}
HK_DEV void set_pos_a(Dyn &B, int b, v2 c, float a) {
  place_a(B.cx, b, c.x);
  place_a(B.cy, b, c.y);
  place_a(B.a, b, a);
}
HK_DEV void set_pos_b(Dyn &B, int b, v2 c, float a) {
  place(B.cx, b, c.x);
  place(B.cy, b, c.y);
  place(B.a, b, a);
}

// fixture radii of a pair: fixture A is always a polygon (walls, goals, players); B is a player polygon or
// the puck circle (build_scene checks this layout)
HK_DEV float pair_rA() { return kPolyRadius; }
HK_DEV float pair_rB(int bB) { return bB == B_PK ? SC.fx[F_PK].radius : kPolyRadius; }

// position-phase view of a contact's manifold (read in place from HBM)
struct ManGeo {
  int type, count;
  v2 ln, lp, pt[2];
};
HK_DEV ManGeo man_geo(const Arena &w, int p) {
  const Quad *rec = man_rec(w, SLDS.manslot[p]);
  const Quad q0 = rec[0], q1 = rec[1], q2 = rec[2];
  ManGeo g;
  const int meta = __float_as_int(q0.x);
  g.count = meta & 0xff;
  g.type = meta >> 8;
  g.ln = V(q0.y, q0.z);
  g.lp = V(q0.w, q1.x);
  g.pt[0] = V(q1.y, q1.z);
  g.pt[1] = g.count > 1 ? V(q1.w, q2.x) : V(0.0f, 0.0f);
  return g;
}

// b2ContactSolver constructor for one contact
HK_DEV void fslot_load(FSlot &s, const Arena &w, int p, int warm, int isl, const ManGeo *geo = nullptr) {
  const int pa = SLDS.pbodyA[p], pb = SLDS.pbodyB[p];
  const Quad *rec = man_rec(w, SLDS.manslot[p]);
  int count, type;
  if (geo) {  // the caller holds the record's geometry: no second read of it
    count = geo->count;
    type = geo->type;
  } else {
    const int meta = __float_as_int(rec[0].x);
    count = meta & 0xff;
    type = meta >> 8;
  }
  s.bits = p | (isl << 5) | (pa << 7) | (pb << 11) | (count << 15) | (count << 17) | (type << 19);
  s.fr = SLDS.friction[p];
  s.mA = inv_mass(pa); s.mB = inv_mass(pb); s.iA = inv_inertia(pa); s.iB = inv_inertia(pb);
  s.Kxx = s.Kxy = s.Kyy = 0.0f;
  s.Nxx = s.Nxy = s.Nyy = 0.0f;
  s.nx = s.ny = 0.0f;
  Quad q3 = Quad{0.0f, 0.0f, 0.0f, 0.0f};
  if (warm) q3 = rec[3];
  const float mni[2] = {q3.x, q3.z}, mti[2] = {q3.y, q3.w};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const bool on = j < count;
    s.ni[j] = on && warm ? 1.0f * mni[j] : 0.0f;
    s.ti[j] = on && warm ? 1.0f * mti[j] : 0.0f;
    s.rAx[j] = s.rAy[j] = s.rBx[j] = s.rBy[j] = 0.0f;
    s.nm[j] = s.tm[j] = s.bias[j] = 0.0f;
  }
  s.sn[0] = s.sn[1] = s.sn[2] = s.sn[3] = 0u;
}

// InitializeVelocityConstraints for one contact (geo: the contact's manifold geometry where the caller already
// holds it, else it is read from the record here)
HK_DEV void fslot_init_velocity(FSlot &s, const Arena &w, const ManGeo *geo = nullptr) {
  const Dyn &B = w.d;
  const float mA = s.mA, mB = s.mB, iA = s.iA, iB = s.iB;
  const int bA = fs_bA(s), bB = fs_bB(s), p = fs_pair(s);
  const float rAr = pair_rA(), rBr = pair_rB(bB);
  v2 cA, cB, vA, vB;
  float aA, aB, wA, wB;
  get_pos_a(B, bA, cA, aA);
  get_pos_b(B, bB, cB, aB);
  get_vel_a(B, bA, vA, wA);
  get_vel_b(B, bB, vB, wB);
  xform xA, xB;
  if (bA >= 3) {  // static body: angle +0, rot_set(+0) == (+0, 1)
    xA.q.s = 0.0f;
    xA.q.c = 1.0f;
  } else {
    xA.q = rot_set(aA);
  }
  xB.q = rot_set(aB);
  xA.p = vsub(cA, mul_rv(xA.q, local_center(bA)));
  xB.p = vsub(cB, mul_rv(xB.q, local_center(bB)));
  // b2WorldManifold::Initialize
  const ManGeo m = geo ? *geo : man_geo(w, p);
  v2 normal, pts[2];
  if (m.type == 1) {
    normal = mul_rv(xA.q, m.ln);
    v2 plane = mul_xv(xA, m.lp);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      v2 clip = mul_xv(xB, m.pt[i]);
      v2 ca = vadd(clip, vs(rAr - dot(vsub(clip, plane), normal), normal));
      v2 cb = vsub(clip, vs(rBr, normal));
      pts[i] = vs(0.5f, vadd(ca, cb));
    }
  } else {
    normal = mul_rv(xB.q, m.ln);
    v2 plane = mul_xv(xB, m.lp);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      v2 clip = mul_xv(xA, m.pt[i]);
      v2 cb = vadd(clip, vs(rBr - dot(vsub(clip, plane), normal), normal));
      v2 ca = vsub(clip, vs(rAr, normal));
      pts[i] = vs(0.5f, vadd(ca, cb));
    }
    normal = vneg(normal);
  }
  s.nx = normal.x;
  s.ny = normal.y;
  const float re = SLDS.restitution[p];
  const int vcount = fs_vcount(s);
  HK_EV(EV_INIT, 1);
  HK_EV(EV_INIT_PT, vcount);
  HK_EV(EV_INIT_BLOCK, vcount == 2);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < vcount) {
      v2 rA = vsub(pts[j], cA), rB = vsub(pts[j], cB);
      s.rAx[j] = rA.x; s.rAy[j] = rA.y; s.rBx[j] = rB.x; s.rBy[j] = rB.y;
      float rnA = crs(rA, normal), rnB = crs(rB, normal);
      float kN = mA + mB + iA * rnA * rnA + iB * rnB * rnB;
      s.nm[j] = kN > 0.0f ? 1.0f / kN : 0.0f;
      v2 tangent = crs_vs(normal, 1.0f);
      float rtA = crs(rA, tangent), rtB = crs(rB, tangent);
      float kT = mA + mB + iA * rtA * rtA + iB * rtB * rtB;
      s.tm[j] = kT > 0.0f ? 1.0f / kT : 0.0f;
      s.bias[j] = 0.0f;
      float vRel = dot(normal, vsub(vsub(vadd(vB, crs_sv(wB, rB)), vA), crs_sv(wA, rA)));
      if (vRel < -kVelocityThreshold) s.bias[j] = -re * vRel;
    }
  }
  if (vcount == 2) {
    v2 r1A = V(s.rAx[0], s.rAy[0]), r1B = V(s.rBx[0], s.rBy[0]);
    v2 r2A = V(s.rAx[1], s.rAy[1]), r2B = V(s.rBx[1], s.rBy[1]);
    float rn1A = crs(r1A, normal), rn1B = crs(r1B, normal);
    float rn2A = crs(r2A, normal), rn2B = crs(r2B, normal);
    float k11 = mA + mB + iA * rn1A * rn1A + iB * rn1B * rn1B;
    float k22 = mA + mB + iA * rn2A * rn2A + iB * rn2B * rn2B;
    float k12 = mA + mB + iA * rn1A * rn2A + iB * rn1B * rn2B;
    if (k11 * k11 < 1000.0f * (k11 * k22 - k12 * k12)) {
      s.Kxx = k11; s.Kxy = k12; s.Kyy = k22;
      float a = s.Kxx, b = s.Kxy, c = s.Kxy, d = s.Kyy;
      float det = a * d - b * c;
      if (det != 0.0f) det = 1.0f / det;
      s.Nxx = det * d;
      s.Nxy = -det * c;
      s.Nyy = det * a;
    } else {
      s.bits = (s.bits & ~(3 << 15)) | (1 << 15);  // vcount = 1
    }
  }
}

HK_DEV void fslot_warm_start(const FSlot &s, Dyn &B) {
  const int bA = fs_bA(s), bB = fs_bB(s), vcount = fs_vcount(s);
  HK_EV(EV_WARM_PT, vcount);
  v2 vA, vB;
  float wA, wB;
  get_vel_a(B, bA, vA, wA);
  get_vel_b(B, bB, vB, wB);
  const v2 normal = V(s.nx, s.ny), tangent = crs_vs(normal, 1.0f);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < vcount) {
      v2 P = vadd(vs(s.ni[j], normal), vs(s.ti[j], tangent));
      wA -= s.iA * crs(V(s.rAx[j], s.rAy[j]), P);
      vA = vsub(vA, vs(s.mA, P));
      wB += s.iB * crs(V(s.rBx[j], s.rBy[j]), P);
      vB = vadd(vB, vs(s.mB, P));
    }
  }
  set_vel_a(B, bA, vA, wA);
  set_vel_b(B, bB, vB, wB);
}

// one b2ContactSolver::SolveVelocityConstraints pass over one contact (tangent rows, then the normal row or the
// 2-point block solver), on the two bodies' velocities held in locals; the 2-vector arithmetic is packed fp32
// relative velocity at a contact point, dv = vB + wB x rB - vA - wA x rA (Box2D's operation order)
template <bool kSA>
HK_DEV f2 rel_vel(f2 vA, float wA, f2 vB, float wB, f2 rA, f2 rB) {
  if constexpr (kSA) return (vB + bc(wB) * perp(rB)) - bc(0.0f) * perp(rA);
  else return ((vB + bc(wB) * perp(rB)) - vA) - bc(wA) * perp(rA);
}

// (f2) with Box2D's float operations in Box2D's order.
// kSA: body A is static, so vA = wA = +0 at every solve (the callers reset them) and A's updates are dead.
// The relative velocity then keeps only the operations that can change a bit: u - (+0) == u for every u,
// but u - (+0)*perp(rA) can turn a -0 of u into +0, so that product stays (loop-invariant, hoisted).
// kP: the manifold's point count when the caller knows it for every lane running the call (1 or 2), else 0
// (read per lane): a wave whose lanes all solve one-point contacts skips the block solver's code entirely.
template <bool kSA = false, int kP = 0>
HK_DEV void fslot_solve_velocity_p(FSlot &s, f2 &vA, float &wA, f2 &vB, float &wB) {
  const float mA = s.mA, iA = s.iA, mB = s.mB, iB = s.iB;
  const int vcount = kP ? kP : fs_vcount(s);
  HK_EV(vcount == 1 ? EV_VEL1 : EV_VEL2, 1);
  const f2 normal = f2{s.nx, s.ny}, tangent = f2{1.0f * s.ny, -1.0f * s.nx};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < vcount) {
      const f2 rA = f2{s.rAx[j], s.rAy[j]}, rB = f2{s.rBx[j], s.rBy[j]};
      const f2 dv = rel_vel<kSA>(vA, wA, vB, wB, rA, rB);
      float vt = pdot(dv, tangent) - 0.0f;
      float lambda = s.tm[j] * (-vt);
      float maxF = s.fr * s.ni[j];
      float newI = fclamp(s.ti[j] + lambda, -maxF, maxF);
      lambda = newI - s.ti[j];
      s.ti[j] = newI;
      const f2 P = bc(lambda) * tangent;
      if constexpr (!kSA) {
        vA = vA - bc(mA) * P;
        wA -= iA * pcrs(rA, P);
      }
      vB = vB + bc(mB) * P;
      wB += iB * pcrs(rB, P);
    }
  }
  if (vcount == 1) {
    const f2 rA = f2{s.rAx[0], s.rAy[0]}, rB = f2{s.rBx[0], s.rBy[0]};
    const f2 dv = rel_vel<kSA>(vA, wA, vB, wB, rA, rB);
    float vn = pdot(dv, normal);
    float lambda = -s.nm[0] * (vn - s.bias[0]);
    float newI = fmax2(s.ni[0] + lambda, 0.0f);
    lambda = newI - s.ni[0];
    s.ni[0] = newI;
    const f2 P = bc(lambda) * normal;
    if constexpr (!kSA) {
      vA = vA - bc(mA) * P;
      wA -= iA * pcrs(rA, P);
    }
    vB = vB + bc(mB) * P;
    wB += iB * pcrs(rB, P);
  } else {
    const f2 r1A = f2{s.rAx[0], s.rAy[0]}, r1B = f2{s.rBx[0], s.rBy[0]};
    const f2 r2A = f2{s.rAx[1], s.rAy[1]}, r2B = f2{s.rBx[1], s.rBy[1]};
    v2 a = V(s.ni[0], s.ni[1]);
    const f2 dv1 = rel_vel<kSA>(vA, wA, vB, wB, r1A, r1B);
    const f2 dv2 = rel_vel<kSA>(vA, wA, vB, wB, r2A, r2B);
    float vn1 = pdot(dv1, normal), vn2 = pdot(dv2, normal);
    v2 b;
    b.x = vn1 - s.bias[0];
    b.y = vn2 - s.bias[1];
    b = vsub(b, V(s.Kxx * a.x + s.Kxy * a.y, s.Kxy * a.x + s.Kyy * a.y));
    // Box2D's four cases (both points / point 1 only / point 2 only / none), first one that holds wins.  All four
    // candidates are computed and the winner picked by selects: the same float operations as the if-cascade, without
    // its exec-mask juggling -- the cascade's short blocks were issued predicated anyway (r06, -DHK_ASM_MARKS dump).
    const v2 x1 = vneg(V(s.Nxx * b.x + s.Nxy * b.y, s.Nxy * b.x + s.Nyy * b.y));
    const float x2x = -s.nm[0] * b.x, vn2c = s.Kxy * x2x + b.y;  // case 2: x = (x2x, 0)
    const float x3y = -s.nm[1] * b.y, vn1c = s.Kxy * x3y + b.x;  // case 3: x = (0, x3y)
    const bool ok1 = (x1.x >= 0.0f) & (x1.y >= 0.0f);
    const bool ok2 = (x2x >= 0.0f) & (vn2c >= 0.0f);
    const bool ok3 = (x3y >= 0.0f) & (vn1c >= 0.0f);
    const bool ok4 = (b.x >= 0.0f) & (b.y >= 0.0f);  // case 4: x = (0, 0)
    v2 x;
    x.x = ok1 ? x1.x : (ok2 ? x2x : 0.0f);
    x.y = ok1 ? x1.y : ((!ok2 & ok3) ? x3y : 0.0f);
    const bool ok = ok1 | ok2 | ok3 | ok4;
    (void)vn1;
    (void)vn2;
    if (ok) {
      const v2 d = vsub(x, a);
      const f2 P1 = bc(d.x) * normal, P2 = bc(d.y) * normal;
      if constexpr (!kSA) {
        vA = vA - bc(mA) * (P1 + P2);
        wA -= iA * (pcrs(r1A, P1) + pcrs(r2A, P2));
      }
      vB = vB + bc(mB) * (P1 + P2);
      wB += iB * (pcrs(r1B, P1) + pcrs(r2B, P2));
      s.ni[0] = x.x;
      s.ni[1] = x.y;
    }
  }
}

template <int kP = 0>
HK_DEV void fslot_solve_velocity(FSlot &s, Dyn &B) {
  const int bA = fs_bA(s), bB = fs_bB(s);
  v2 vA, vB;
  float wA, wB;
  get_vel_a(B, bA, vA, wA);
  get_vel_b(B, bB, vB, wB);
  f2 pA = F2(vA), pB = F2(vB);
  fslot_solve_velocity_p<false, kP>(s, pA, wA, pB, wB);
  set_vel_a(B, bA, V2(pA), wA);
  set_vel_b(B, bB, V2(pB), wB);
}

// one NGS position pass over one contact (b2ContactSolver::SolvePositionConstraints body).  In this scene
// SolveTOIPositionConstraints' mass gating is the identity (see solve_toi), so one routine serves both.
// The 2-vector arithmetic is packed (f2): the same float operations in the same order as the scalar form.
HK_DEV float fslot_solve_position(const FSlot &s, Arena &w, float baum, float minSep, const ManGeo &m) {
  HK_MARK(posrow_begin);
  Dyn &B = w.d;
  const float mA = s.mA, mB = s.mB, iA = s.iA, iB = s.iB;
  const int bA = fs_bA(s), bB = fs_bB(s), pcount = fs_pcount(s);
  HK_EV(EV_POS_PT, pcount);
  const f2 lcA = F2(local_center(bA)), lcB = F2(local_center(bB));
  const float rAr = pair_rA(), rBr = pair_rB(bB);
  v2 cA0, cB0;
  float aA, aB;
  get_pos_a(B, bA, cA0, aA);
  get_pos_b(B, bB, cB0, aB);
  f2 cA = F2(cA0), cB = F2(cB0);
  const f2 ln = F2(m.ln), lp = F2(m.lp);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < pcount) {
      rot qA, qB;
      // a static body stays at angle +0 (iA == 0 keeps aA bit-exact), and rot_set(+0) == (+0, 1)
      if (bA >= 3) {
        qA.s = 0.0f;
        qA.c = 1.0f;
      } else {
        qA = rot_set(aA);
      }
      qB = rot_set(aB);
      const f2 pA = cA - prv(qA, lcA), pB = cB - prv(qB, lcB);
      f2 normal, point;
      float sep;
      if (m.type == 1) {
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
      float C = fclamp(baum * (sep + kLinearSlop), -kMaxLinearCorrection, 0.0f);
      float rnA = pcrs(rA, normal), rnB = pcrs(rB, normal);
      float K = mA + mB + iA * rnA * rnA + iB * rnB * rnB;
      float impulse = K > 0.0f ? -C / K : 0.0f;
      const f2 P = bc(impulse) * normal;
      cA = cA - bc(mA) * P;
      aA -= iA * pcrs(rA, P);
      cB = cB + bc(mB) * P;
      aB += iB * pcrs(rB, P);
    }
  }
  if (bA < 3) set_pos_a(B, bA, V2(cA), aA);
  set_pos_b(B, bB, V2(cB), aB);
  HK_MARK(posrow_end);
  return minSep;
}

// ------------------------------------------------------------------------------------------------
// Slot files.  Both run fn(slot, i) over the first nc slots in order (Gauss-Seidel order matters).
//   RegSlots<C>: C slots in registers, loops fully unrolled (compile-time slot indices) -- the hot path
//             (islands: C = kIslandC, TOI mini-islands: C = kToiC).
//   HbmSlots: up to kBigC slots in the HBM workspace DevState::ws ([slot][word][arena], lane-contiguous);
//             each visit loads one slot into registers, runs fn and writes it back.  Used by the rare
//             large islands (~1e-5 of arena-steps) so they neither inflate the hot path's register
//             budget nor use private (scratch) memory.
template <int C>
struct RegSlots {
  static constexpr bool kRegister = true;
  static_assert(C >= 2, "the one- and two-contact loops use slots 0 and 1");
  FSlot s[C];
  ManGeo g[C];  // position-phase geometry, loaded once per position loop (load_geo)
  HK_DEV void load_geo(int nc, const Arena &w) {
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (i < nc) g[i] = man_geo(w, fs_pair(s[i]));
  }
  HK_DEV const ManGeo &geo(int i, const FSlot &, const Arena &) const { return g[i]; }
  template <typename Fn>
  HK_DEV void each(int nc, Fn &&fn) {
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (i < nc) fn(s[i], i);
  }
  HK_DEV void set_pair(int nc, int p, int isl) {
#pragma unroll
    for (int q = 0; q < C; ++q) s[q].bits = (q == nc) ? (p | (isl << 5)) : s[q].bits;
  }
};

struct HbmSlots {
  static constexpr bool kRegister = false;
  float *ws;
  int64_t n, a;
  HK_DEV float &word(int i, int k) const { return ws[((int64_t)i * kSlotWords + k) * n + a]; }
  template <typename Fn>
  HK_DEV void each(int nc, Fn &&fn) {
#pragma unroll 1
    for (int i = 0; i < nc; ++i) {
      FSlot t;
      float tw[kSlotWords];
#pragma unroll
      for (int k = 0; k < kSlotWords; ++k) tw[k] = word(i, k);
      __builtin_memcpy(&t, tw, sizeof(FSlot));
      fn(t, i);
      __builtin_memcpy(tw, &t, sizeof(FSlot));
#pragma unroll
      for (int k = 0; k < kSlotWords; ++k) word(i, k) = tw[k];
    }
  }
  HK_DEV void set_pair(int nc, int p, int isl) {
    if (nc < kBigC) word(nc, (int)(offsetof(FSlot, bits) / 4)) = __int_as_float(p | (isl << 5));
  }
  HK_DEV void load_geo(int, const Arena &) {}
  HK_DEV ManGeo geo(int, const FSlot &s, const Arena &w) const { return man_geo(w, fs_pair(s)); }
};
template <typename SL> struct SlotCap;
template <int C> struct SlotCap<RegSlots<C>> { static constexpr int value = C; };
template <> struct SlotCap<HbmSlots> { static constexpr int value = kBigC; };

// per-lane exchange of register slots i (compile-time) and j (runtime, j >= i), word by word through selects.
// The words are copied out and back with memcpy (no type-punned pointer: strict-aliasing clean on the host and
// sanitizer builds; SROA keeps every word in a register on the device).
template <int C>
HK_DEV void slot_swap(RegSlots<C> &S, int i, int j) {
  static_assert(sizeof(FSlot) == kSlotWords * 4, "FSlot is kSlotWords words");
  uint32_t a[kSlotWords];
  __builtin_memcpy(a, &S.s[i], sizeof(FSlot));
#pragma unroll
  for (int q = 0; q < C; ++q) {
    if (q <= i) continue;
    uint32_t b[kSlotWords];
    __builtin_memcpy(b, &S.s[q], sizeof(FSlot));
    const bool sw = j == q;
#pragma unroll
    for (int k = 0; k < kSlotWords; ++k) {
      const uint32_t x = a[k], y = b[k];
      a[k] = sw ? y : x;
      b[k] = sw ? x : y;
    }
    __builtin_memcpy(&S.s[q], b, sizeof(FSlot));
  }
  __builtin_memcpy(&S.s[i], a, sizeof(FSlot));
}

}  // namespace hk
#include "hk_velocity.h"  // the velocity-loop families and the wave dispatch over the slot files above
namespace hk {

HK_DEV void fslot_store(const FSlot &s, Arena &w) {  // b2ContactSolver::StoreImpulses (j < pointCount)
  float *q3 = reinterpret_cast<float *>(man_rec(w, SLDS.manslot[fs_pair(s)]) + 3);
  const int vcount = fs_vcount(s);
  if (vcount == 2) {
    *reinterpret_cast<Quad *>(q3) = Quad{s.ni[0], s.ti[0], s.ni[1], s.ti[1]};
  } else if (vcount == 1) {
    q3[0] = s.ni[0];
    q3[1] = s.ti[0];
  }
}

HK_DEV void integrate_one(float h, Dyn &B, int b) {
  v2 c = V(B.cx[b], B.cy[b]), v = V(B.vx[b], B.vy[b]);
  float a = B.a[b], wv = B.w[b];
  v2 tr = vs(h, v);
  if (dot(tr, tr) > kMaxTranslation * kMaxTranslation) {
    float ratio = kMaxTranslation / vlen(tr);
    v = vs(ratio, v);
  }
  float rotn = h * wv;
  if (rotn * rotn > kMaxRotation * kMaxRotation) {
    float ratio = kMaxRotation / fabs2(rotn);
    wv *= ratio;
  }
  c = vadd(c, vs(h, v));
  a += h * wv;
  B.cx[b] = c.x; B.cy[b] = c.y; B.a[b] = a; B.vx[b] = v.x; B.vy[b] = v.y; B.w[b] = wv;
}

}  // namespace hk

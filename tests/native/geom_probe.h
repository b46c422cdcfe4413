/* geom_probe.h -- one record layout and one per-case function for each primitive of hk_geom.h (gjk_distance,
 * time_of_impact, collide_polygons, collide_poly_circle).  TEST INFRASTRUCTURE ONLY: the product never loads it.
 *
 * Three builds fill the same records (tests/geom_cases.py holds the numpy dtypes):
 *   geom_probe.hip        one lane per case on gfx950, built with the step library's own flags
 *   geom_probe_host.cpp   the same header under g++ (like hostcheck)
 *   geom_probe_oracle.c   oracle/hk_oracle.c's static functions of the same names
 * The C part below (records) is shared by all three; the C++ part (GP_WITH_HK) is written against hk_geom.h.
 *
 * Every record is made of 4-byte words.  Outputs are normalised so that every word is defined: simplex-cache
 * index pairs at and beyond `count` are -1; a manifold with count == 0 is all zero but for `count`; point 1 of a
 * one-point manifold is zero.  (Manifold::ni / ti are not written by the collide functions and are not recorded.) */
#ifndef GEOM_PROBE_H
#define GEOM_PROBE_H
#include <stdint.h>

#define GP_MAXV 8
#define GP_NSCENE 13 /* fixtures of the compiled-in scene, F_WT ... F_PK */

typedef struct {
  int32_t circle, count;
  float radius, pad;
  float vx[GP_MAXV], vy[GP_MAXV], nx[GP_MAXV], ny[GP_MAXV];
} GpFixture; /* 36 words */

typedef struct { int32_t fA, fB; float xa[4], xb[4]; } GpPoseCase; /* transforms as raw (px, py, s, c); 10 words */
typedef struct { float lcx, lcy, c0x, c0y, cx, cy, a0, a; } GpSweep;
typedef struct { int32_t fA, fB; GpSweep sA, sB; float tMax; } GpToiCase; /* 19 words */

typedef struct { float dist, dist_radii, metric; int32_t count; int32_t iA[3], iB[3]; } GpDistOut; /* 10 words */
typedef struct { int32_t state; float t; } GpToiOut;                                             /* 2 words */
typedef struct {
  int32_t type, count;
  float lnx, lny, lpx, lpy;
  float p0x, p0y, p1x, p1y;
  uint32_t id0, id1;
} GpManOut; /* 12 words */

#if defined(__cplusplus) && defined(GP_WITH_HK)
/* ---- written once against hk_geom.h; instantiates what the product instantiates (hk_collide.h, hk_world.h):
 * TOI: Proxy<kStaticVerts, true> against Proxy<kMaxPolyVerts>; distance: test_overlap's Proxy<kStaticVerts> against
 * Proxy<kMaxPolyVerts>; manifolds: RFix<kStaticVerts> or RFix<kMaxPolyVerts> for A (by A's vertex count, as the
 * product picks by the body being static), RFix<kMaxPolyVerts> or RFix<1> for B. */
namespace gp {
using namespace hk;

HK_DEV Fixture to_fixture(const GpFixture &g) {
  Fixture f;
  f.circle = g.circle; f.count = g.count; f.body = 0; f.sensor = 0;
#pragma unroll
  for (int k = 0; k < kMaxPolyVerts; ++k) { f.vx[k] = g.vx[k]; f.vy[k] = g.vy[k]; f.nx[k] = g.nx[k]; f.ny[k] = g.ny[k]; }
  f.radius = g.radius; f.friction = 0.0f; f.restitution = 0.0f; f.pad = 0.0f;
  return f;
}
HK_DEV xform to_xform(const float *x) { xform t; t.p = V(x[0], x[1]); t.q.s = x[2]; t.q.c = x[3]; return t; }
HK_DEV Sweep to_sweep(const GpSweep &g) {
  Sweep s;
  s.lc = V(g.lcx, g.lcy); s.c0 = V(g.c0x, g.c0y); s.c = V(g.cx, g.cy); s.a0 = g.a0; s.a = g.a; s.alpha0 = 0.0f;
  return s;
}

HK_DEV void distance_case(const GpFixture *fx, const GpPoseCase &c, GpDistOut &o) {
  const Fixture fA = to_fixture(fx[c.fA]), fB = to_fixture(fx[c.fB]);
  const Proxy<kStaticVerts> pA = make_proxy<kStaticVerts>(fA);
  const Proxy<kMaxPolyVerts> pB = make_proxy<kMaxPolyVerts>(fB);
  const xform xA = to_xform(c.xa), xB = to_xform(c.xb);
  SimplexCache cache;
  cache.count = 0; cache.metric = 0.0f;
  o.dist = gjk_distance(cache, pA, xA, pB, xB, 0);
  o.metric = cache.metric;
  o.count = cache.count;
#pragma unroll
  for (int k = 0; k < 3; ++k) { o.iA[k] = k < cache.count ? cache.iA[k] : -1; o.iB[k] = k < cache.count ? cache.iB[k] : -1; }
  SimplexCache c2;
  c2.count = 0; c2.metric = 0.0f;
  o.dist_radii = gjk_distance(c2, pA, xA, pB, xB, 1);
}

HK_DEV void toi_case(const GpFixture *fx, const GpToiCase &c, GpToiOut &o) {
  const Fixture fA = to_fixture(fx[c.fA]), fB = to_fixture(fx[c.fB]);
  const Proxy<kStaticVerts, true> pA = make_proxy<kStaticVerts, true>(fA);
  const Proxy<kMaxPolyVerts> pB = make_proxy<kMaxPolyVerts>(fB);
  float t = 0.0f;
  o.state = time_of_impact(pA, pB, to_sweep(c.sA), to_sweep(c.sB), c.tMax, t);
  o.t = t;
}

HK_DEV void manifold_out(const Manifold &m, GpManOut &o) {
  const bool any = m.count > 0, two = m.count > 1;
  o.count = m.count;
  o.type = any ? m.type : 0;
  o.lnx = any ? m.ln.x : 0.0f; o.lny = any ? m.ln.y : 0.0f;
  o.lpx = any ? m.lp.x : 0.0f; o.lpy = any ? m.lp.y : 0.0f;
  o.p0x = any ? m.pt_lp[0].x : 0.0f; o.p0y = any ? m.pt_lp[0].y : 0.0f;
  o.p1x = two ? m.pt_lp[1].x : 0.0f; o.p1y = two ? m.pt_lp[1].y : 0.0f;
  o.id0 = any ? m.id[0] : 0u;
  o.id1 = two ? m.id[1] : 0u;
}

HK_DEV void manifold_case(const GpFixture *fx, const GpPoseCase &c, GpManOut &o) {
  const Fixture fA = to_fixture(fx[c.fA]), fB = to_fixture(fx[c.fB]);
  const xform xA = to_xform(c.xa), xB = to_xform(c.xb);
  Manifold m;
  m.count = 0; m.type = 0;
  m.ln = m.lp = m.pt_lp[0] = m.pt_lp[1] = V(0.0f, 0.0f);
  m.id[0] = m.id[1] = 0u;
  const bool quadA = fA.count <= kStaticVerts;
  if (fB.circle) {
    const RFix<1> cB = load_fix<1>(fB);
    if (quadA) collide_poly_circle(m, load_fix<kStaticVerts>(fA), xA, cB, xB);
    else collide_poly_circle(m, load_fix<kMaxPolyVerts>(fA), xA, cB, xB);
  } else {
    const RFix<kMaxPolyVerts> pB = load_fix<kMaxPolyVerts>(fB);
    if (quadA) collide_polygons(m, load_fix<kStaticVerts>(fA), xA, pB, xB);
    else collide_polygons(m, load_fix<kMaxPolyVerts>(fA), xA, pB, xB);
  }
  manifold_out(m, o);
}

/* the compiled-in scene's fixtures, and per fixture {static body origin x, y, dynamic body local centre x, y} */
inline void scene_export(const Scene &sc, GpFixture *out, float *body4) {
  for (int i = 0; i < NF; ++i) {
    const Fixture &f = sc.fx[i];
    GpFixture &g = out[i];
    g.circle = f.circle; g.count = f.count; g.radius = f.radius; g.pad = 0.0f;
    for (int k = 0; k < kMaxPolyVerts; ++k) { g.vx[k] = f.vx[k]; g.vy[k] = f.vy[k]; g.nx[k] = f.nx[k]; g.ny[k] = f.ny[k]; }
    const bool dyn = f.body < 3;
    body4[4 * i + 0] = dyn ? 0.0f : sc.spx[f.body];
    body4[4 * i + 1] = dyn ? 0.0f : sc.spy[f.body];
    body4[4 * i + 2] = dyn ? sc.lcx[f.body] : 0.0f;
    body4[4 * i + 3] = dyn ? sc.lcy[f.body] : 0.0f;
  }
}
}  // namespace gp
#endif

#endif

/* geom_probe_oracle.c -- geom_probe.h's records filled from the CPU oracle's own static gjk_distance,
 * time_of_impact, collide_polygons and collide_poly_circle (test infrastructure only; built by tests/geom_cases.py
 * next to the oracle library, with the oracle's flags).  Exports gp_*; every other symbol is the oracle's own. */
#include "../../oracle/hk_oracle.c"

#include "geom_probe.h"

static fixture gp_fixture(const GpFixture *g) {
  fixture f;
  memset(&f, 0, sizeof(f));
  f.circle = g->circle;
  f.count = g->count;
  f.radius = g->radius;
  for (int k = 0; k < MAX_POLY_VERTS; ++k) { f.v[k] = V(g->vx[k], g->vy[k]); f.n[k] = V(g->nx[k], g->ny[k]); }
  return f;
}
static xform gp_xform(const float *x) { xform t; t.p = V(x[0], x[1]); t.q.s = x[2]; t.q.c = x[3]; return t; }
static sweep gp_sweep(const GpSweep *g) {
  sweep s;
  s.lc = V(g->lcx, g->lcy); s.c0 = V(g->c0x, g->c0y); s.c = V(g->cx, g->cy); s.a0 = g->a0; s.a = g->a; s.alpha0 = 0.0f;
  return s;
}
static int gp_bad(int fA, int fB, int nfx) { return fA < 0 || fA >= nfx || fB < 0 || fB >= nfx; }

void gp_scene(GpFixture *out, float *body4) {
  init_scene();
  for (int i = 0; i < NF; ++i) {
    const fixture *f = &SCENE.fx[i];
    GpFixture *g = &out[i];
    memset(g, 0, sizeof(*g));
    g->circle = f->circle; g->count = f->count; g->radius = f->radius;
    for (int k = 0; k < MAX_POLY_VERTS; ++k) {
      g->vx[k] = f->v[k].x; g->vy[k] = f->v[k].y; g->nx[k] = f->n[k].x; g->ny[k] = f->n[k].y;
    }
    const body *b = &SCENE.proto[f->body];
    body4[4 * i + 0] = b->dynamic ? 0.0f : b->xf.p.x;
    body4[4 * i + 1] = b->dynamic ? 0.0f : b->xf.p.y;
    body4[4 * i + 2] = b->dynamic ? b->lc.x : 0.0f;
    body4[4 * i + 3] = b->dynamic ? b->lc.y : 0.0f;
  }
}

int gp_distance(const GpFixture *fx, int nfx, const GpPoseCase *c, GpDistOut *o, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (gp_bad(c[i].fA, c[i].fB, nfx)) return -1;
    const fixture fA = gp_fixture(&fx[c[i].fA]), fB = gp_fixture(&fx[c[i].fB]);
    const proxy pA = make_proxy(&fA), pB = make_proxy(&fB);
    const xform xA = gp_xform(c[i].xa), xB = gp_xform(c[i].xb);
    simplex_cache cache;
    memset(&cache, 0, sizeof(cache));
    o[i].dist = gjk_distance(&cache, &pA, xA, &pB, xB, 0, NULL, NULL);
    o[i].metric = cache.metric;
    o[i].count = cache.count;
    for (int k = 0; k < 3; ++k) {
      o[i].iA[k] = k < cache.count ? cache.iA[k] : -1;
      o[i].iB[k] = k < cache.count ? cache.iB[k] : -1;
    }
    simplex_cache c2;
    memset(&c2, 0, sizeof(c2));
    o[i].dist_radii = gjk_distance(&c2, &pA, xA, &pB, xB, 1, NULL, NULL);
  }
  return 0;
}

int gp_toi(const GpFixture *fx, int nfx, const GpToiCase *c, GpToiOut *o, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (gp_bad(c[i].fA, c[i].fB, nfx)) return -1;
    const fixture fA = gp_fixture(&fx[c[i].fA]), fB = gp_fixture(&fx[c[i].fB]);
    const proxy pA = make_proxy(&fA), pB = make_proxy(&fB);
    float t = 0.0f;
    o[i].state = time_of_impact(&pA, &pB, gp_sweep(&c[i].sA), gp_sweep(&c[i].sB), c[i].tMax, &t);
    o[i].t = t;
  }
  return 0;
}

int gp_manifold(const GpFixture *fx, int nfx, const GpPoseCase *c, GpManOut *o, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (gp_bad(c[i].fA, c[i].fB, nfx)) return -1;
    const fixture fA = gp_fixture(&fx[c[i].fA]), fB = gp_fixture(&fx[c[i].fB]);
    const xform xA = gp_xform(c[i].xa), xB = gp_xform(c[i].xb);
    manifold m;
    memset(&m, 0, sizeof(m));
    if (fB.circle) collide_poly_circle(&m, &fA, xA, &fB, xB);
    else collide_polygons(&m, &fA, xA, &fB, xB);
    GpManOut *r = &o[i];
    memset(r, 0, sizeof(*r));
    r->count = m.count;
    if (m.count > 0) {
      r->type = m.type;
      r->lnx = m.ln.x; r->lny = m.ln.y; r->lpx = m.lp.x; r->lpy = m.lp.y;
      r->p0x = m.pt[0].lp.x; r->p0y = m.pt[0].lp.y; r->id0 = m.pt[0].id;
    }
    if (m.count > 1) { r->p1x = m.pt[1].lp.x; r->p1y = m.pt[1].lp.y; r->id1 = m.pt[1].id; }
  }
  return 0;
}

// hk_render.h -- the picture of an arena as a per-pixel coverage law (hockey/hockey_env.py:697-744 render,
// drawlist :303-319, :414), one source for gfx950 (hk_render.hip) and the host (hostcheck/hk_render_host.cpp).
//
// Native pixel units u = 60 x, v = 60 y (SCALE), y up, frame 600 x 480.  Pixel (row i from the top, column j) of an
// H x W image samples (u, v) = ((j + 0.5) 600 / W, 480 - (i + 0.5) 480 / H) and takes the colour of the LAST shape
// in draw order that covers the sample, white otherwise:
//    1 circle (300, 240) r 100 grey     2 circle (50, 240) r 75 goal orange    3 box 60..160 x 140..340 white
//    4 circle (550, 240) r 75 orange    5 box 440..540 x 140..340 white        6, 7 boxes 50..550 x 440..460, 20..40 black
//    8-11 the four goal-post walls, black    12 player 1 racket    13 player 2 racket    14 puck, circle r 13, black
// A polygon covers a point whose signed Euclidean distance to it is <= 1 px (pygame's fill plus the width-2 outline
// in the same colour); a circle covers a point within its radius (its outline is drawn inward).  A racket is
// RACKETPOLY x 1.2 (x negated for player 2) rotated by the body's angle about the body ORIGIN and translated to
// 60 (x, y): the pose words of hk_get_state, not the centre of mass.  The goal sensors are not in drawlist.  A body
// whose pose has a non-finite component is not drawn (the puck's pose is its position: a circle has no angle to
// draw, and hk_set_state rows carry NaN there).
//
// Everything is float32 with -ffp-contract=off and IEEE division, and the rotation is hk_core.h's rot_set, so the
// host build and the gfx950 build give the same bytes (tests/test_gpu_render.py).  tests/render_ref.py states the
// same law in float64 from signed distances; the two differ only at knife-edge pixels (tests/test_render_law.py).
#pragma once
#include "hk_core.h"

namespace hkr {

enum { PAL_WHITE = 0, PAL_GREY, PAL_GOAL, PAL_BLACK, PAL_P1, PAL_P2, PAL_N };
constexpr int kRacketVerts = 7;
constexpr float kNativeW = 600.0f, kNativeH = 480.0f, kScale = 60.0f;
constexpr float kPuckRadius = 13.0f;
constexpr float kBoxMargin = 1.0625f;  // the 1 px polygon dilation plus room for float32 rounding
constexpr int kQuadPixels = 4;         // a lane owns 4 horizontally consecutive pixels
constexpr int kTileLanes = 256;        // lanes of a workgroup
constexpr int kTileRepeat = 8;         // a workgroup owns a tile of kTileLanes * kTileRepeat quads of one frame

// a racket in pixel units: vertices a[k], edges e[k] = a[k+1] - a[k], 1 / |e[k]|^2, outward unit normals n[k], the
// dilated bounding box
struct Racket {
  float ax[kRacketVerts], ay[kRacketVerts], ex[kRacketVerts], ey[kRacketVerts], inv[kRacketVerts];
  float nx[kRacketVerts], ny[kRacketVerts];
  float bb[4];  // min u, min v, max u, max v
  int valid;
};
struct Puck {
  float cx, cy, bb[4];
  int valid;
};
struct Frame {
  Racket r[2];
  Puck pk;
};

__host__ HK_DEV uint32_t palette_rgb(uint32_t k) {  // r | g << 8 | b << 16, by selects (no table in memory)
  uint32_t c = 0x00ffffffu;                         // 0 white
  c = k == PAL_GREY ? 0x00ccccccu : c;              // (204, 204, 204)
  c = k == PAL_GOAL ? 0x008acbefu : c;              // (239, 203, 138)
  c = k == PAL_BLACK ? 0x00000000u : c;
  c = k == PAL_P1 ? 0x003562ebu : c;                // (235, 98, 53)
  c = k == PAL_P2 ? 0x00c79e5du : c;                // (93, 158, 199)
  return c;
}

HK_DEV bool finite_f(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

HK_DEV float sample_u(int j, float su) { return ((float)j + 0.5f) * su; }
HK_DEV float sample_v(int i, float sv) { return kNativeH - ((float)i + 0.5f) * sv; }

// one edge of a convex polygon: the side of the sample (cross product) and its squared distance to the segment
HK_DEV void edge_test(float ax, float ay, float ex, float ey, float inv, float u, float v, bool &pos, bool &neg,
                      float &best) {
  const float dx = u - ax, dy = v - ay;
  const float c = ex * dy - ey * dx;
  pos = pos && (c >= 0.0f);
  neg = neg && (c <= 0.0f);
  float t = (dx * ex + dy * ey) * inv;
  t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  const float qx = dx - t * ex, qy = dy - t * ey;
  const float d2 = qx * qx + qy * qy;
  best = d2 < best ? d2 : best;
}

// Which of the 4 samples (u[p], v) the racket covers (signed distance <= 1 px), bit p for pixel p.  Most samples are
// settled by their offsets from the edge lines along the outward normals alone: inside (largest offset <= 0) or
// more than 1 px outside some edge line; only the 1-px ring around the polygon, where corners round the dilated
// outline, needs the distance to the boundary.  Edges run in the outer loop, so an edge's words are read once for
// the 4 pixels.
HK_DEV uint32_t racket_quad(const Racket &R, const float *u, float v) {
  float h[kQuadPixels];
#pragma unroll
  for (int p = 0; p < kQuadPixels; p++) h[p] = -hk::kFltMax;
#pragma unroll
  for (int k = 0; k < kRacketVerts; k++) {
    const float nx = R.nx[k], ny = R.ny[k], ax = R.ax[k], ay = R.ay[k];
    const float hv = ny * (v - ay);
#pragma unroll
    for (int p = 0; p < kQuadPixels; p++) {
      const float hn = nx * (u[p] - ax) + hv;
      h[p] = hn > h[p] ? hn : h[p];
    }
  }
  uint32_t covered = 0, ring = 0;
#pragma unroll
  for (int p = 0; p < kQuadPixels; p++) {
    covered |= (h[p] <= 0.0f ? 1u : 0u) << p;
    ring |= (h[p] > 0.0f && h[p] <= 1.0f ? 1u : 0u) << p;
  }
  if (ring) {
    float best[kQuadPixels];
#pragma unroll
    for (int p = 0; p < kQuadPixels; p++) best[p] = hk::kFltMax;
#pragma unroll
    for (int k = 0; k < kRacketVerts; k++) {
      const float ax = R.ax[k], ay = R.ay[k], ex = R.ex[k], ey = R.ey[k], inv = R.inv[k];
      bool pos = true, neg = true;
#pragma unroll
      for (int p = 0; p < kQuadPixels; p++) edge_test(ax, ay, ex, ey, inv, u[p], v, pos, neg, best[p]);
    }
#pragma unroll
    for (int p = 0; p < kQuadPixels; p++) covered |= (best[p] <= 1.0f ? 1u : 0u) << p & ring;
  }
  return covered;
}

// a static quad, either winding: inside (on one side of every edge), or within 1 px of the boundary
HK_DEV bool quad_covers(const float *P, float u, float v) {  // P = x0, y0, ..., x3, y3
  bool pos = true, neg = true;
  float best = hk::kFltMax;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int n = (k + 1) & 3;
    const float ex = P[2 * n] - P[2 * k], ey = P[2 * n + 1] - P[2 * k + 1];
    edge_test(P[2 * k], P[2 * k + 1], ex, ey, 1.0f / (ex * ex + ey * ey), u, v, pos, neg, best);
  }
  return pos || neg || best <= 1.0f;
}

HK_DEV bool circle_covers(float cx, float cy, float r, float u, float v) {
  const float dx = u - cx, dy = v - cy;
  return dx * dx + dy * dy <= r * r;
}

// shapes 1-11 at one sample point
HK_DEV uint32_t static_index(float u, float v) {
  // boxes 3, 5, 6, 7 and the goal-post walls 8-11 (poly (-10, 135), (10, 128), (10, -5), (-10, -5) about
  // (55, 450) y negated, (55, 30), (545, 450) x and y negated, (545, 30) x negated), as absolute pixel quads
  const float box3[8] = {60, 140, 160, 140, 160, 340, 60, 340};
  const float box5[8] = {440, 140, 540, 140, 540, 340, 440, 340};
  const float wall6[8] = {50, 440, 550, 440, 550, 460, 50, 460};
  const float wall7[8] = {50, 20, 550, 20, 550, 40, 50, 40};
  const float post8[8] = {45, 315, 65, 322, 65, 455, 45, 455};
  const float post9[8] = {45, 165, 65, 158, 65, 25, 45, 25};
  const float post10[8] = {555, 315, 535, 322, 535, 455, 555, 455};
  const float post11[8] = {555, 165, 535, 158, 535, 25, 555, 25};
  uint32_t k = PAL_WHITE;
  k = circle_covers(300.0f, 240.0f, 100.0f, u, v) ? PAL_GREY : k;
  k = circle_covers(50.0f, 240.0f, 75.0f, u, v) ? PAL_GOAL : k;
  k = quad_covers(box3, u, v) ? PAL_WHITE : k;
  k = circle_covers(550.0f, 240.0f, 75.0f, u, v) ? PAL_GOAL : k;
  k = quad_covers(box5, u, v) ? PAL_WHITE : k;
  const bool black = quad_covers(wall6, u, v) || quad_covers(wall7, u, v) || quad_covers(post8, u, v) ||
                     quad_covers(post9, u, v) || quad_covers(post10, u, v) || quad_covers(post11, u, v);
  return black ? PAL_BLACK : k;
}

// the palette indices of pixels j0 .. j0+3 of row i under shapes 1-11, one per byte, pixel j0 in the low byte
HK_DEV uint32_t static_quad(int i, int j0, float su, float sv) {
  const float v = sample_v(i, sv);
  uint32_t q = 0;
#pragma unroll
  for (int p = 0; p < kQuadPixels; p++) q |= static_index(sample_u(j0 + p, su), v) << (8 * p);
  return q;
}

// a racket's pose in pixel units from its state words s = x, y, angle (hk_get_state: the body origin)
struct Pose {
  float px, py;
  hk::rot q;
  bool ok;
};
HK_DEV Pose racket_pose(const float *s) {
  const float x = s[0], y = s[1];
  float a = s[2];
  Pose P;
  P.px = kScale * x;
  P.py = kScale * y;
  // a body a million pixels away covers no sample of the frame either way: keep the arithmetic finite
  P.ok = finite_f(x) && finite_f(y) && finite_f(a) && P.px > -1.0e6f && P.px < 1.0e6f && P.py > -1.0e6f &&
         P.py < 1.0e6f;
  if (!P.ok) a = P.px = P.py = 0.0f;
  // rot_set reduces by multiples of pi/2 in float32, good for a few hundred turns; beyond that reduce by whole
  // turns in float64 first (the same operations on both builds)
  if (a > 1024.0f || a < -1024.0f) {
    const double turn = 6.283185307179586;
    a = (float)((double)a - turn * __builtin_rint((double)a / turn));
  }
  P.q = hk::rot_set(a);
  return P;
}

// vertex k of RACKETPOLY x 1.2 (hockey_env.py:31-32; x negated for player 2) under the pose
HK_DEV void racket_vertex(const Pose &P, int player, int k, float &wx, float &wy) {
  // x: -12, 6, 6, -12, -21.6, -25.2, -21.6    y: 24, 24, -24, -24, -12, 0, 12   (selects: no table in memory)
  float vx = (k == 1 || k == 2) ? 6.0f : -12.0f;
  vx = (k == 4 || k == 6) ? -21.6f : vx;
  vx = k == 5 ? -25.2f : vx;
  float vy = k < 2 ? 24.0f : -24.0f;
  vy = k == 4 ? -12.0f : vy;
  vy = k == 5 ? 0.0f : vy;
  vy = k == 6 ? 12.0f : vy;
  vx = player ? -vx : vx;
  wx = (P.q.c * vx - P.q.s * vy) + P.px;
  wy = (P.q.s * vx + P.q.c * vy) + P.py;
}

// vertex k, edge k -> k+1 and its outward unit normal (player 1's polygon runs clockwise, player 2's mirror image
// counter-clockwise; a rotation keeps that).  One lane per edge on the GPU.
HK_DEV void setup_racket_edge(const float *s, int player, int k, Racket &R) {
  const Pose P = racket_pose(s);
  float ax, ay, bx, by;
  racket_vertex(P, player, k, ax, ay);
  racket_vertex(P, player, k + 1 == kRacketVerts ? 0 : k + 1, bx, by);
  const float ex = bx - ax, ey = by - ay;
  const float l2 = ex * ex + ey * ey, len = sqrtf(l2);
  const float sg = player ? 1.0f : -1.0f;
  R.ax[k] = ax;
  R.ay[k] = ay;
  R.ex[k] = ex;
  R.ey[k] = ey;
  R.inv[k] = 1.0f / l2;
  R.nx[k] = (sg * ey) / len;
  R.ny[k] = (-sg * ex) / len;
}

// the dilated bounding box, and whether the racket is drawn at all
HK_DEV void setup_racket_box(const float *s, int player, Racket &R) {
  const Pose P = racket_pose(s);
  float mnx = hk::kFltMax, mny = hk::kFltMax, mxx = -hk::kFltMax, mxy = -hk::kFltMax;
#pragma unroll
  for (int k = 0; k < kRacketVerts; k++) {
    float wx, wy;
    racket_vertex(P, player, k, wx, wy);
    mnx = wx < mnx ? wx : mnx;
    mny = wy < mny ? wy : mny;
    mxx = wx > mxx ? wx : mxx;
    mxy = wy > mxy ? wy : mxy;
  }
  R.bb[0] = mnx - kBoxMargin;
  R.bb[1] = mny - kBoxMargin;
  R.bb[2] = mxx + kBoxMargin;
  R.bb[3] = mxy + kBoxMargin;
  R.valid = P.ok ? 1 : 0;
}

HK_DEV void setup_puck(const float *s, Puck &P) {  // s = x, y of the puck
  const float x = s[0], y = s[1];
  const float px = kScale * x, py = kScale * y;
  const bool ok = finite_f(x) && finite_f(y) && px > -1.0e6f && px < 1.0e6f && py > -1.0e6f && py < 1.0e6f;
  P.cx = ok ? px : 0.0f;
  P.cy = ok ? py : 0.0f;
  P.bb[0] = P.cx - (kPuckRadius + 0.0625f);
  P.bb[1] = P.cy - (kPuckRadius + 0.0625f);
  P.bb[2] = P.cx + (kPuckRadius + 0.0625f);
  P.bb[3] = P.cy + (kPuckRadius + 0.0625f);
  P.valid = ok ? 1 : 0;
}

HK_DEV void setup_frame(const float *state18, Frame &F) {  // the host's order; the kernel spreads it over lanes
  for (int b = 0; b < 2; b++) {
    for (int k = 0; k < kRacketVerts; k++) setup_racket_edge(state18 + 6 * b, b, k, F.r[b]);
    setup_racket_box(state18 + 6 * b, b, F.r[b]);
  }
  setup_puck(state18 + 12, F.pk);
}

HK_DEV bool span_meets(const float *bb, float u0, float u3, float v) {
  return u3 >= bb[0] && u0 <= bb[2] && v >= bb[1] && v <= bb[3];
}

// shapes 12-14 over the background indices bg4 of pixels j0 .. j0+3 of row i
HK_DEV uint32_t dynamic_quad(const Frame &F, uint32_t bg4, int i, int j0, float su, float sv) {
  const float v = sample_v(i, sv);
  float u[kQuadPixels];
#pragma unroll
  for (int p = 0; p < kQuadPixels; p++) u[p] = sample_u(j0 + p, su);
  uint32_t q = bg4;
#pragma unroll
  for (int b = 0; b < 2; b++) {
    const Racket &R = F.r[b];
    if (R.valid && span_meets(R.bb, u[0], u[kQuadPixels - 1], v)) {
      const uint32_t covered = racket_quad(R, u, v);
#pragma unroll
      for (int p = 0; p < kQuadPixels; p++)
        if (covered >> p & 1u) q = (q & ~(0xffu << (8 * p))) | ((uint32_t)(PAL_P1 + b) << (8 * p));
    }
  }
  if (F.pk.valid && span_meets(F.pk.bb, u[0], u[kQuadPixels - 1], v)) {
#pragma unroll
    for (int p = 0; p < kQuadPixels; p++)
      if (circle_covers(F.pk.cx, F.pk.cy, kPuckRadius, u[p], v))
        q = (q & ~(0xffu << (8 * p))) | ((uint32_t)PAL_BLACK << (8 * p));
  }
  return q;
}

// 4 palette indices -> the 12 bytes r g b r g b ... as three little-endian dwords
HK_DEV void quad_rgb(uint32_t q, uint32_t &d0, uint32_t &d1, uint32_t &d2) {
  const uint32_t c0 = palette_rgb(q & 0xffu), c1 = palette_rgb((q >> 8) & 0xffu), c2 = palette_rgb((q >> 16) & 0xffu),
                 c3 = palette_rgb(q >> 24);
  d0 = c0 | (c1 << 24);
  d1 = (c1 >> 8) | (c2 << 16);
  d2 = (c2 >> 16) | (c3 << 8);
}

}  // namespace hkr

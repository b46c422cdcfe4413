// hk_game.h -- the game around world.Step: HockeyEnv.step's pre-solve laws, observations, info, reward and
// BasicOpponent.
#pragma once
#include "hk_body.h"

namespace hk {

// ------------------------------------------------------------------------------------------------
// HockeyEnv.step laws (hockey_env.py:420-483, 610-633), numpy NEP-50 + pybox2d float32 semantics
// ------------------------------------------------------------------------------------------------
constexpr double kDtPy = 0.02;  // self.timeStep = 1.0 / FPS  (hockey_env.py:119)
constexpr double kPiD = 3.141592653589793;

template <int B>
HK_DEV void check_boundaries(Arena &w, float &f0, float &f1, int one) {
  const double px = w.d.px[B], py = w.d.py[B];
  if ((one && px < 1.5 && f0 < 0) || (!one && px > 8.5 && f0 > 0) || (one && px > 5.0 && f0 > 0) ||
      (!one && px < 5.0 && f0 < 0)) {
    float vel0 = w.d.vx[B];
    if (w.vel_ref) { w.d.vx[B] = 0.0f; vel0 = 0.0f; }
    f0 = -vel0;
  }
  if ((py > 8.0 - 1.2 && f1 > 0) || (py < 1.2 && f1 < 0)) {
    float vel1 = w.d.vy[B];
    if (w.vel_ref) { w.d.vy[B] = 0.0f; vel1 = 0.0f; }
    f1 = -vel1;
  }
}

template <int B>
HK_DEV void translation_law(Arena &w, float a0, float a1) {
  constexpr int one = (B == B_P1);
  const double vx = w.d.vx[B], vy = w.d.vy[B];
  const double speed = sqrt(vx * vx + vy * vy);
  float f0, f1;
  if (one) { f0 = a0 * 6000.0f; f1 = a1 * 6000.0f; }
  else { f0 = (-a0) * 6000.0f; f1 = (-a1) * 6000.0f; }
  const double px = w.d.px[B], m = SC.mass[B];
  if ((one && px > 5.0 - 0.5) || (!one && px < 5.0 + 0.5)) {
    f0 = 0.0f;
    if (one) {
      if (vx > 0) f0 = (float)((((-2.0) * vx) * m) / kDtPy);
      f0 = f0 + (float)(((((-1.0) * (px - 5.0)) * vx) * m) / kDtPy);
    } else {
      if (vx < 0) f0 = (float)((((-2.0) * vx) * m) / kDtPy);
      f0 = f0 + (float)((((1.0 * (px - 5.0)) * vx) * m) / kDtPy);
    }
    w.d.ld[B] = 20.0f;
    check_boundaries<B>(w, f0, f1, one);
    apply_force<B>(w, V(f0, f1));
    return;
  }
  if (speed < 10.0) {
    w.d.ld[B] = 5.0f;
    check_boundaries<B>(w, f0, f1, one);
    apply_force<B>(w, V(f0, f1));
  } else {
    w.d.ld[B] = 20.0f;
    const float mf = (float)m;
    const float d0 = (0.02f * f0) / mf, d1 = (0.02f * f1) / mf;
    const double nx = vx + (double)d0, ny = vy + (double)d1;
    if (sqrt(nx * nx + ny * ny) < speed) {
      check_boundaries<B>(w, f0, f1, one);
      apply_force<B>(w, V(f0, f1));
    }
  }
}

template <int B>
HK_DEV void rotation_law(Arena &w, float a) {
  const double ang = w.d.a[B], wv = w.d.w[B], m = SC.mass[B];
  if (fabs(ang) > kPiD / 3) {
    double t = 0.0;
    if (ang * wv > 0) t = (((-0.1) * wv) * m) / kDtPy;
    t = t + (((-0.1) * ang) * m) / kDtPy;
    w.d.ad[B] = 10.0f;
    apply_torque<B>(w, (float)t);
  } else {
    w.d.ad[B] = 2.0f;
    apply_torque<B>(w, a * 400.0f);
  }
}

template <int B>
HK_DEV void shoot(Arena &w) {
  const double ca = hk_cos((double)w.d.a[B]), sa = hk_sin((double)w.d.a[B]);
  const double sgn = B == B_P1 ? 1.0 : -1.0;
  v2 f = V((float)(ca * sgn), (float)(sa * sgn));
  const float m = SC.mass[B_PK];
  f = V(f.x * m, f.y * m);
  f = V(f.x / 0.02f, f.y / 0.02f);
  f = V(f.x * 60.0f, f.y * 60.0f);
  apply_force<B_PK>(w, f);
}

template <int B>
HK_DEV void keep_puck(Arena &w) {
  set_transform<B_PK>(w, V(w.d.px[B], w.d.py[B]), w.d.a[B_PK]);
  set_linear_velocity<B_PK>(w, V(w.d.vx[B], w.d.vy[B]));
}

HK_DEV float clip1(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }

HK_DEV void presolve(Arena &w, const float *a8) {
  float a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = clip1(a8[i]);
  translation_law<B_P1>(w, a[0], a[1]);
  rotation_law<B_P1>(w, a[2]);
  translation_law<B_P2>(w, a[4], a[5]);
  rotation_law<B_P2>(w, a[6]);
  {
    const double vx = w.d.vx[B_PK], vy = w.d.vy[B_PK];
    const double s = sqrt(vx * vx + vy * vy);
    w.d.ld[B_PK] = s > 25.0 ? 10.0f : 0.05f;
  }
  if (w.keep_mode) {
    if (w.has1 > 1) {
      keep_puck<B_P1>(w);
      w.has1 -= 1;
      if (w.has1 == 1 || a[3] > 0.5f) { shoot<B_P1>(w); w.has1 = 0; }
    }
    if (w.has2 > 1) {
      keep_puck<B_P2>(w);
      w.has2 -= 1;
      if (w.has2 == 1 || a[7] > 0.5f) { shoot<B_P2>(w); w.has2 = 0; }
    }
  }
}

HK_DEV void observe(const Arena &w, float *o) {
  const Dyn &d = w.d;
  o[0] = d.px[0] - 5.0f; o[1] = d.py[0] - 4.0f; o[2] = d.a[0];
  o[3] = d.vx[0]; o[4] = d.vy[0]; o[5] = d.w[0];
  o[6] = d.px[1] - 5.0f; o[7] = d.py[1] - 4.0f; o[8] = d.a[1];
  o[9] = d.vx[1]; o[10] = d.vy[1]; o[11] = d.w[1];
  o[12] = d.px[2] - 5.0f; o[13] = d.py[2] - 4.0f;
  o[14] = d.vx[2]; o[15] = d.vy[2];
  o[16] = w.keep_mode ? (float)w.has1 : 0.0f;
  o[17] = w.keep_mode ? (float)w.has2 : 0.0f;
}

HK_DEV void observe_two(const Arena &w, float *o) {
  const Dyn &d = w.d;
  o[0] = -(d.px[1] - 5.0f); o[1] = -(d.py[1] - 4.0f); o[2] = d.a[1];
  o[3] = -d.vx[1]; o[4] = -d.vy[1]; o[5] = d.w[1];
  o[6] = -(d.px[0] - 5.0f); o[7] = -(d.py[0] - 4.0f); o[8] = d.a[0];
  o[9] = -d.vx[0]; o[10] = -d.vy[0]; o[11] = d.w[0];
  o[12] = -(d.px[2] - 5.0f); o[13] = -(d.py[2] - 4.0f);
  o[14] = -d.vx[2]; o[15] = -d.vy[2];
  o[16] = w.keep_mode ? (float)w.has2 : 0.0f;
  o[17] = w.keep_mode ? (float)w.has1 : 0.0f;
}

// _get_info / get_info_agent_two (hockey_env.py:542-591), double like the reference
template <int TWO>
HK_DEV void info_side(const Arena &w, double *info4) {
  constexpr int me = TWO ? B_P2 : B_P1;
  const Dyn &d = w.d;
  const double T = (double)w.max_t;
  double close = 0.0;
  const int cond = TWO ? ((double)d.px[2] > 5.0 && (double)d.vx[2] >= 0) : ((double)d.px[2] < 5.0 && (double)d.vx[2] <= 0);
  if (cond) {
    const float dx = d.px[me] - d.px[2], dy = d.py[me] - d.py[2];
    const double dd = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
    const double max_dist = 250.0 / 60.0;
    const double factor = -30.0 / ((max_dist * T) / 2);
    close = close + dd * factor;
  }
  const double touch = ((TWO ? w.has2 : w.has1) == 15) ? 1.0 : 0.0;
  const double f2 = TWO ? (-1.0) / (T * 25) : 1.0 / (T * 25);
  info4[0] = TWO ? -w.winner : w.winner;
  info4[1] = close;
  info4[2] = touch;
  info4[3] = (double)d.vx[2] * f2;
}

HK_DEV double compute_reward(const Arena &w) {
  double r = 0;
  if (w.done) {
    if (w.winner == 1) r += 10;
    else if (w.winner != 0) r -= 10;
  }
  return r;
}

// BasicOpponent.act (hockey_env.py:787-833) on an own-frame float32 obs, double arithmetic
HK_DEV void basic_opponent(int weak, int keep_mode, double &phase, double inc, const float *of, float *act) {
  const double p1x = of[0], p1y = of[1], p1a = of[2];
  const double v1[3] = {of[3], of[4], of[5]};
  const double pkx = of[12], pky = of[13], pvx = of[14], pvy = of[15];
  double tx, ty;
  phase += inc;
  const double kp = weak ? 0.5 : 10.0, kd = 0.5;
  if (pvx < 30.0 / 60.0) {
    const double dx = p1x - pkx, dy = p1y - pky;
    const double dist = sqrt(dx * dx + dy * dy);
    double ady = p1y - pky;
    if (ady < 0) ady = -ady;
    if (p1x < pkx && ady < 30.0 / 60.0) {
      tx = pkx + 0.2;
      ty = pky + (pvy * dist) * 0.1;
    } else {
      tx = -210.0 / 60.0;
      ty = pky;
    }
  } else {
    tx = -210.0 / 60.0;
    ty = 0.0;
  }
  const double ta = (kPiD / 3) * hk_sin(phase);
  const double o16 = of[16];
  const double shoot_ = (keep_mode && o16 > 0 && o16 < 7) ? 1.0 : 0.0;
  const double err[3] = {tx - p1x, ty - p1y, ta - p1a};
  const double gains[3] = {kp, kp / 5, kp / 2};
  const double tb[3] = {0.1, 0.1, 0.1 * 10};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double q = err[i] / (v1[i] + 0.01);
    if (q < 0) q = -q;
    const double nb = (q < tb[i]) ? 1.0 : 0.0;
    const double x = err[i] * gains[i] - (v1[i] * nb) * kd;
    act[i] = (float)(x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x));
  }
  act[3] = (float)shoot_;
}

}  // namespace hk

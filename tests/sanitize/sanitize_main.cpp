// Sanitizer build of the CPU-side code (ASan/UBSan on host code): the oracle (oracle/hk_oracle.c)
// and the kernel's per-lane source compiled for the host (hostcheck), both under
// -fsanitize=address,undefined, stepped in lockstep over every mode and policy kind, then over the non-finite
// scenarios of tests/nonfinite_cases.py.  Test infrastructure
// only; tests/test_sanitize.py builds and runs it (make -C tests/sanitize).  Exit status 0 = no sanitizer
// report and every step bit-identical; GPU code is not sanitized (GPU ASan is not available on the pool).
#include "../../hockey-env_amd/csrc/hostcheck/hk_hostcheck.cpp"

extern "C" {
#include "../../oracle/hk_oracle.h"
}

#include <cstdio>
#include <random>

static const int kPol[][2] = {{3, 3}, {1, 1}, {0, 2}, {2, 0}};

// ---- second pass: values that are not finite numbers (include/hockey.h "Non-finite values"), the scenarios of
// tests/nonfinite_cases.py restated.  Action and increment scenarios: lockstep on all arenas, final state and the
// counters the oracle keeps.  State-borne scenarios: lockstep on the unaffected arenas, then on all arenas after a
// masked reset of the affected ones.
static const int64_t kN = 128;
static const int kLanes[5] = {0, 5, 63, 64, 127};
static const int kClean = 10, kAffected = 60;
static float f32_of(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }
static double f64_of(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

struct Lockstep {
  int64_t n;
  void *h;
  hkov *v;
  std::vector<float> o1, o2, p1, p2, r1, r2, q1, q2, i1, i2, j1, j2, f1, f2, a1, a2;
  std::vector<uint8_t> d1, d2;
  Lockstep(int mode, int pol0, int pol1, int auto_reset, uint64_t seed)
      : n(kN), o1(n * 18), o2(n * 18), p1(n * 18), p2(n * 18), r1(n), r2(n), q1(n), q2(n), i1(n * 4), i2(n * 4),
        j1(n * 4), j2(n * 4), f1(n * 18), f2(n * 18), a1(n * 8), a2(n * 8), d1(n), d2(n) {
    const int cfg7[7] = {1, mode, auto_reset, 0, pol0, pol1, 0};
    const int32_t cfg6[6] = {1, mode, auto_reset, 0, pol0, pol1};
    h = hkh_create(n, cfg7, seed, 0);
    hkh_reset(h, nullptr, nullptr, nullptr, nullptr);
    v = hkov_create(n, cfg6, seed, 0);
  }
  ~Lockstep() {
    hkh_destroy(h);
    hkov_destroy(v);
  }
  template <class T>
  static bool rows_equal(const std::vector<T> &a, const std::vector<T> &b, int64_t k, const uint8_t *skip, int64_t n) {
    for (int64_t r = 0; r < n; ++r)
      if (!(skip && skip[r]) && memcmp(&a[r * k], &b[r * k], k * sizeof(T))) return false;
    return true;
  }
  // one step of both; true when every output row outside `skip` (nullable) is bit-identical
  bool step(const float *act, const double *inc, const uint8_t *mix, const uint8_t *skip) {
    StepIO io{};
    io.actions = act;
    io.opp_inc = inc;
    io.obs = o1.data(); io.obs2 = p1.data(); io.reward = r1.data(); io.reward2 = q1.data(); io.done = d1.data();
    io.info = i1.data(); io.info2 = j1.data(); io.final_obs = f1.data(); io.actions_out = a1.data();
    io.policy2 = mix;
    hkh_step(h, &io);
    hkov_step(v, act, inc, o2.data(), p2.data(), r2.data(), q2.data(), d2.data(), i2.data(), j2.data(), a2.data(),
              f2.data(), mix);
    return rows_equal(o1, o2, 18, skip, n) && rows_equal(p1, p2, 18, skip, n) && rows_equal(r1, r2, 1, skip, n) &&
           rows_equal(q1, q2, 1, skip, n) && rows_equal(d1, d2, 1, skip, n) && rows_equal(i1, i2, 4, skip, n) &&
           rows_equal(j1, j2, 4, skip, n) && rows_equal(f1, f2, 18, skip, n) && rows_equal(a1, a2, 8, skip, n);
  }
  bool state_equal(const uint8_t *skip) {
    std::vector<float> s1(n * 18), s2(n * 18);
    std::vector<int32_t> x1(n * 5), x2(n * 5);
    hkh_get_state(h, s1.data(), x1.data());
    hkov_get_state(v, s2.data(), x2.data());
    return rows_equal(s1, s2, 18, skip, n) && rows_equal(x1, x2, 5, skip, n);
  }
  // counters 0..4 equal and HK_CNT_BAD_ACTION of both equal to `want`
  bool counters_equal(int64_t want) {
    unsigned long long c[16];
    int64_t oc[16];
    hkh_counters(h, c);
    hkov_counters(v, oc);
    for (int k = 0; k < 5; ++k)
      if ((int64_t)c[k] != oc[k]) return false;
    return (int64_t)c[9] == want && oc[9] == want;
  }
};

static int nonfinite_external_pass() {
  static const uint32_t kAct[9] = {0x7FC00000u, 0xFFC00000u, 0x7FA12345u, 0x7F800000u, 0xFF800000u,
                                   0x7F61B1E6u /* 3e38 */, 0xFF61B1E6u, 0x00000001u, 0x80000000u};
  static const uint64_t kInc[4] = {0x7FF8000000000000ull, 0xFFF4000000012345ull, 0x7FF0000000000000ull,
                                   0xFFF0000000000000ull};
  // {policy 1, policy 2, io.actions given, per-step mix}; rows 0..2 the action kinds, 3..5 the increment kinds
  static const int kKind[6][4] = {{0, 0, 1, 0}, {0, 3, 1, 0}, {0, 0, 1, 1}, {3, 2, 0, 0}, {0, 3, 1, 0}, {0, 0, 1, 1}};
  int bad = 0;
  for (int mode = 0; mode < 3; ++mode)
    for (int kind = 0; kind < 6; ++kind) {
      const bool incs = kind >= 3;
      for (int val = 0; val < (incs ? 4 : 9); ++val) {
        Lockstep L(mode, kKind[kind][0], kKind[kind][1], 1, 31 + mode);
        std::mt19937 rng(mode * 100 + kind * 10 + val);
        std::uniform_real_distribution<float> U(-1.2f, 1.2f);
        std::uniform_real_distribution<double> UI(0.0, 0.2);
        std::vector<float> act(kN * 8);
        std::vector<double> inc(kN * 2);
        std::vector<uint8_t> p2(kN);
        const int c0 = (val + mode) % 2 ? 3 : 0;  // components 0..4 or 3..7 over the five affected arenas
        const bool counted = incs || val < 3;
        bool ok = true;
        for (int t = 0; t < kClean + kAffected && ok; ++t) {
          for (auto &x : act) x = U(rng);
          for (auto &x : inc) x = UI(rng);
          for (auto &x : p2) x = (uint8_t)(rng() % 3 == 0 ? 0 : 2 + rng() % 2);
          if (t >= kClean)
            for (int j = 0; j < 5; ++j) {
              if (incs) inc[kLanes[j] * 2 + j % 2] = f64_of(kInc[val]);
              else act[kLanes[j] * 8 + (c0 + j) % 8] = f32_of(kAct[val]);
            }
          ok = L.step(kKind[kind][2] ? act.data() : nullptr, incs ? inc.data() : nullptr,
                      kKind[kind][3] ? p2.data() : nullptr, nullptr);
        }
        ok = ok && L.state_equal(nullptr) && L.counters_equal(counted ? 5 * kAffected : 0);
        if (!ok) {
          std::printf("non-finite %s: mismatch: mode %d kind %d value %d\n", incs ? "increment" : "action", mode, kind, val);
          ++bad;
        }
      }
    }
  return bad;
}

static int nonfinite_state_pass() {
  const float inf = f32_of(0x7F800000u), nan = f32_of(0x7FC00000u);
  struct Poke { int k; float v; };
  struct Case { const char *name; bool params; std::vector<Poke> pokes; };
  // state18 = p1 {x, y, angle, vx, vy, w}, p2 {...}, puck {...}; params6 = p2x, p2y, puckx, pucky, puck_fx, puck_fy
  const std::vector<Case> cases = {
      {"p1_x_+inf", false, {{0, inf}}},          {"puck_y_-inf", false, {{13, -inf}}},
      {"p2_xy_inf", false, {{6, inf}, {7, -inf}}}, {"p1_angle_+inf", false, {{2, inf}}},
      {"puck_vx_+inf", false, {{15, inf}}},      {"p1_vx_-inf", false, {{3, -inf}}},
      {"p2_w_+inf", false, {{11, inf}}},         {"puck_v_3e38", false, {{15, 3e38f}, {16, 3e38f}}},
      {"p2_v_-3e38", false, {{9, -3e38f}, {10, 3e38f}}},
      {"all_v_3e38", false, {{3, 3e38f}, {4, -3e38f}, {5, 3e38f}, {9, 3e38f}, {15, -3e38f}}},
      {"param_puckx_nan", true, {{2, nan}}},     {"param_p2y_+inf", true, {{1, inf}}},
      {"param_force_-inf", true, {{4, -inf}}},   {"param_force_nan", true, {{4, nan}, {5, nan}}}};
  int bad = 0;
  for (const Case &c : cases) {
    Lockstep L(0, 0, 0, 0, 7);
    std::mt19937 rng(77);
    std::uniform_real_distribution<float> U(-1.2f, 1.2f);
    std::vector<float> act(kN * 8), st(kN * 18), prm(kN * 6);
    std::vector<uint8_t> hit(kN, 0);
    for (int j = 0; j < 5; ++j) hit[kLanes[j]] = 1;
    bool ok = true;
    auto steps = [&](int k, const uint8_t *skip) {
      for (int t = 0; t < k && ok; ++t) {
        for (auto &x : act) x = U(rng);
        ok = L.step(act.data(), nullptr, nullptr, skip) && L.state_equal(skip);
      }
    };
    steps(kClean, nullptr);
    if (c.params) {
      for (int64_t a = 0; a < kN; ++a) {
        const float p6[6] = {7.0f + 0.01f * (a % 7), 4.0f, 3.0f, 4.0f + 0.02f * (a % 5), 0.0f, 0.0f};
        std::memcpy(&prm[a * 6], p6, sizeof(p6));
        for (const Poke &p : c.pokes) prm[a * 6 + p.k] = p.v;
      }
      hkh_reset(L.h, hit.data(), prm.data(), nullptr, nullptr);
      hkov_reset(L.v, hit.data(), prm.data(), nullptr, nullptr);
    } else {
      hkh_get_state(L.h, st.data(), nullptr);
      for (int64_t a = 0; a < kN; ++a)
        for (const Poke &p : c.pokes) st[a * 18 + p.k] = p.v;
      hkh_set_state(L.h, hit.data(), st.data(), nullptr);
      hkov_set_state(L.v, hit.data(), st.data(), nullptr);
    }
    steps(kAffected, hit.data());
    hkh_reset(L.h, hit.data(), nullptr, nullptr, nullptr);  // device placement: the episode words agree (no auto-reset)
    hkov_reset(L.v, hit.data(), nullptr, nullptr, nullptr);
    steps(kAffected, nullptr);
    if (!ok) {
      std::printf("non-finite state: mismatch: %s\n", c.name);
      ++bad;
    }
  }
  return bad;
}

int main() {
  int bad = 0;
  for (int mode = 0; mode < 3; ++mode) {
    for (const auto &pol : kPol) {
      const int64_t n = 48;
      const int cfg7[7] = {1, mode, 1, 0, pol[0], pol[1], 0};
      const int32_t cfg6[6] = {1, mode, 1, 0, pol[0], pol[1]};
      void *h = hkh_create(n, cfg7, 11 + mode, 100);
      hkh_reset(h, nullptr, nullptr, nullptr, nullptr);
      hkov *v = hkov_create(n, cfg6, 11 + mode, 100);
      std::mt19937 rng(mode * 10 + pol[0]);
      std::uniform_real_distribution<float> U(-1.2f, 1.2f);
      std::vector<float> act(n * 8), o1(n * 18), o2(n * 18), r1(n), r2(n), i1(n * 4), i2(n * 4), fo1(n * 18),
          fo2(n * 18);
      std::vector<uint8_t> d1(n), d2(n), p2(n);
      for (int t = 0; t < 260; ++t) {
        for (auto &x : act) x = U(rng);
        for (auto &x : p2) x = (uint8_t)(rng() % 3 == 0 ? 0 : 2 + rng() % 2);
        const uint8_t *mix = (t % 2) ? p2.data() : nullptr;
        StepIO io{};
        io.actions = act.data();
        io.obs = o1.data();
        io.reward = r1.data();
        io.done = d1.data();
        io.info = i1.data();
        io.final_obs = fo1.data();
        io.policy2 = mix;
        hkh_step(h, &io);
        hkov_step(v, act.data(), nullptr, o2.data(), nullptr, r2.data(), nullptr, d2.data(), i2.data(), nullptr,
                  nullptr, fo2.data(), mix);
        if (memcmp(o1.data(), o2.data(), o1.size() * 4) || memcmp(r1.data(), r2.data(), r1.size() * 4) ||
            memcmp(d1.data(), d2.data(), d1.size()) || memcmp(i1.data(), i2.data(), i1.size() * 4) ||
            memcmp(fo1.data(), fo2.data(), fo1.size() * 4)) {
          std::printf("mismatch: mode %d policies %d/%d step %d\n", mode, pol[0], pol[1], t);
          ++bad;
          break;
        }
      }
      hkh_destroy(h);
      hkov_destroy(v);
    }
  }
  bad += nonfinite_external_pass();
  bad += nonfinite_state_pass();
  std::printf("sanitized lockstep: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}

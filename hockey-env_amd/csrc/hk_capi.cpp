// hk_capi.cpp -- the extern "C" boundary declared in include/hockey.h.
//
// Owns the per-context device state (SoA arrays in HBM, allocated once at hk_create and sized for the
// whole arena batch), validates arguments, and launches the gfx950 kernels on the caller's stream.
// Errors are reported as negative status codes plus a thread-local message (hk_last_error); no C++
// exception crosses the ABI.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hockey.h"
#include "hk_arena_copy.h"
#include "hk_host_step.h"
#include "hk_kernels.h"

namespace {
thread_local std::string g_err;
}

int hk::fail(int code, const char *fmt, const char *a, long long b) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), fmt, a, b);
  g_err = buf;
  return code;
}

int hk::hipfail(hipError_t e, const char *where) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), "%s: %s", where, hipGetErrorString(e));
  g_err = buf;
  return HK_E_HIP;
}

namespace {

using hk::fail;
using hk::hipfail;

struct Ctx {
  int device = 0;
  hk::DevState s{};
  hk::KCfg cfg{};
  hk::HostStep hs;  // hk_step_host's buffer and resident step server (hk_host_step.h)
  // hk_reset_seeded's scratch: the placement kernel's params [N,6] and puck sides [N], read by the reset launch
  // that follows it on the same stream (allocated at hk_create: no allocation on the call path)
  float *seed_params = nullptr;
  uint8_t *seed_one = nullptr;
};

int check_policy(int p) { return p >= HK_POLICY_EXTERNAL && p <= HK_POLICY_BASIC_STRONG; }

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Entry-point prologue: HK_CTX rejects a NULL context and names it `c`; HK_QUIESCED makes its device current and
// stops its step server, so the call never runs beside that server (a server that does not stop in time fails the
// call with HK_E_DEVICE).  HK_ENTER is both; launched() is the epilogue of a call that ends in a launch or copy.
#define HK_CTX(ctx, who)                                               \
  if (!(ctx)) return fail(HK_E_INVALID, "%s: ctx is NULL", who);       \
  Ctx *c = (Ctx *)(ctx)
#define HK_QUIESCED(c, who)                                            \
  DeviceGuard g((c)->device);                                          \
  if (const int q_ = (c)->hs.quiesce(who)) return q_
#define HK_ENTER(ctx, who) \
  HK_CTX(ctx, who);        \
  HK_QUIESCED(c, who)

int launched(hipError_t e, const char *who) { return e == hipSuccess ? HK_OK : hipfail(e, who); }

// The device keeps the BasicOpponent phases as [3][N] (row-major by phase row); the ABI's arrays are [N, rows].
int phase_rows(const char *who, void *ctx, int rows, double *phase_out, const double *phase_in, void *stream) {
  HK_ENTER(ctx, who);
  hipError_t e = hipSuccess;
  for (int r = 0; r < rows && e == hipSuccess && phase_out; ++r)
    e = hipMemcpy2DAsync(phase_out + r, rows * sizeof(double), c->s.phase + (size_t)r * c->s.n, sizeof(double),
                         sizeof(double), c->s.n, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  for (int r = 0; r < rows && e == hipSuccess && phase_in; ++r)
    e = hipMemcpy2DAsync(c->s.phase + (size_t)r * c->s.n, sizeof(double), phase_in + r, rows * sizeof(double),
                         sizeof(double), c->s.n, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return launched(e, who);
}

}  // namespace

extern "C" {

const char *hk_last_error(void) { return g_err.c_str(); }

const char *hk_version(void) { return "hockey-mi355x 0.2 (gfx950, lane-per-arena step kernel)"; }

int hk_create(int device, int64_t n, const hk_config *cfg, void **out) {
  if (!out) return fail(HK_E_INVALID, "hk_create: out is NULL%s", "");
  *out = nullptr;
  if (n <= 0 || n > (int64_t)1 << 30) return fail(HK_E_INVALID, "hk_create: bad n_arenas %s%lld", "", n);
  if (!cfg) return fail(HK_E_INVALID, "hk_create: cfg is NULL%s");
  if (cfg->mode < 0 || cfg->mode > 2) return fail(HK_E_INVALID, "hk_create: bad mode%s");
  if (!check_policy(cfg->policy[0]) || !check_policy(cfg->policy[1]))
    return fail(HK_E_INVALID, "hk_create: bad policy%s");
  if (cfg->diag_flags & ~HK_DIAG_LARGE_ISLANDS) return fail(HK_E_INVALID, "hk_create: unknown diag_flags%s");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(HK_E_DEVICE, "hk_create: no HIP device available%s");
  if (device < 0 || device >= ndev || device >= hk::kMaxDevices)
    return fail(HK_E_DEVICE, "hk_create: device %s%lld out of range", "", device);
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hipfail(e, "hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(HK_E_DEVICE, "hk_create: device arch %s is not gfx950 (MI355X)", prop.gcnArchName);
  DeviceGuard g(device);
  Ctx *c = new Ctx();
  c->device = c->hs.device = device;
  c->cfg.keep_mode = cfg->keep_mode ? 1 : 0;
  c->cfg.mode = cfg->mode;
  c->cfg.auto_reset = cfg->auto_reset ? 1 : 0;
  c->cfg.vel_ref = cfg->vel_ref_semantics ? 1 : 0;
  c->cfg.policy[0] = cfg->policy[0];
  c->cfg.policy[1] = cfg->policy[1];
  c->cfg.seed = cfg->seed;
  c->cfg.arena_offset = cfg->arena_offset;
  c->cfg.diag = cfg->diag_flags;
  c->s.n = n;
  const size_t nf = (size_t)hk::NFF * n, ni = (size_t)hk::NPW * n, nm = (size_t)hk::NSOLID * hk::NMF * n;
  const size_t nw = (size_t)hk::workspace_words_per_arena() * n;
  if ((e = hipMalloc(&c->s.f, nf * 4)) != hipSuccess || (e = hipMalloc(&c->s.i, ni * 4)) != hipSuccess ||
      (e = hipMalloc(&c->s.man, nm * 4)) != hipSuccess || (e = hipMalloc(&c->s.phase, 3 * n * 8)) != hipSuccess ||
      (e = hipMalloc(&c->s.ws, nw * 4)) != hipSuccess || (e = hipMalloc(&c->s.counters, HK_NUM_COUNTERS * 8)) != hipSuccess ||
      (e = hipMalloc(&c->seed_params, (size_t)HK_PARAM_DIM * n * 4)) != hipSuccess ||
      (e = hipMalloc(&c->seed_one, (size_t)n)) != hipSuccess) {
    hk_destroy(c);
    return hipfail(e, "hk_create: hipMalloc");
  }
  if ((e = hipMemset(c->s.counters, 0, HK_NUM_COUNTERS * 8)) != hipSuccess ||
      (e = hipMemset(c->s.man, 0, nm * 4)) != hipSuccess) {
    hk_destroy(c);
    return hipfail(e, "hk_create: hipMemset");
  }
  if ((e = hk::launch_init(c->s, c->cfg, nullptr)) != hipSuccess) {
    hk_destroy(c);
    return hipfail(e, "hk_create: init kernel");
  }
  // HockeyEnv.__init__ ends with reset(one_starts=True) (hockey_env.py:155): device placement
  if ((e = hk::launch_reset(c->s, c->cfg, nullptr, nullptr, nullptr, nullptr, nullptr)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess) {
    hk_destroy(c);
    return hipfail(e, "hk_create: initial reset");
  }
  *out = c;
  return HK_OK;
}

int hk_destroy(void *ctx) {
  if (!ctx) return HK_OK;
  Ctx *c = (Ctx *)ctx;
  DeviceGuard g(c->device);
  // the shared server stream stays for the process's other contexts
  const int rc = c->hs.quiesce("hk_destroy");
  if (!c->hs.release()) {
    // the step server did not stop within the wait limit: a queued or running server kernel can still touch the
    // arrays and the pinned buffer, so they are leaked rather than freed under it
    delete c;
    return rc;
  }
  if (c->s.f) (void)hipFree(c->s.f);
  if (c->s.i) (void)hipFree(c->s.i);
  if (c->s.man) (void)hipFree(c->s.man);
  if (c->s.ws) (void)hipFree(c->s.ws);
  if (c->s.phase) (void)hipFree(c->s.phase);
  if (c->s.counters) (void)hipFree(c->s.counters);
  if (c->seed_params) (void)hipFree(c->seed_params);
  if (c->seed_one) (void)hipFree(c->seed_one);
  delete c;
  return HK_OK;
}

int64_t hk_num_arenas(const void *ctx) { return ctx ? ((const Ctx *)ctx)->s.n : 0; }

int hk_set_policy(void *ctx, int player, int policy) {
  HK_CTX(ctx, "hk_set_policy");
  if (player < 0 || player > 1 || !check_policy(policy)) return fail(HK_E_INVALID, "hk_set_policy: bad args%s");
  HK_QUIESCED(c, "hk_set_policy");  // a running server holds the old configuration
  c->cfg.policy[player] = policy;
  return HK_OK;
}

// The packed int words (hk_kernels.h PW_*) hold has_puck in [0, 255], max_t in [0, 65535], done in {0, 1} and
// winner in {-1, 0, 1}: a caller's per-arena values outside those ranges are rejected before anything is launched
// (HK_E_INVALID).  The arrays are device memory; they are copied to the host on the call's stream for the check
// (reset / set_state are not on the step path).  Only arenas the mask selects are checked.
static int check_ints(const char *who, int64_t n, int cols, const int32_t *dev, const uint8_t *mask_dev,
                      hipStream_t st) {
  std::vector<int32_t> v((size_t)n * cols);
  std::vector<uint8_t> m(mask_dev ? (size_t)n : 0);
  hipError_t e = hipMemcpyAsync(v.data(), dev, v.size() * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && mask_dev) e = hipMemcpyAsync(m.data(), mask_dev, m.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hipfail(e, who);
  for (int64_t a = 0; a < n; ++a) {
    if (mask_dev && !m[a]) continue;
    const int32_t *r = v.data() + a * cols;
    if (cols == 1) {
      if (r[0] < 0 || r[0] > hk::kMaxTMax)
        return fail(HK_E_INVALID, "%s: max_t out of range [0, 65535]", who);
      continue;
    }
    if (r[0] < 0 || r[0] > hk::kHasMax || r[1] < 0 || r[1] > hk::kHasMax)
      return fail(HK_E_INVALID, "%s: aux has_puck out of range [0, 255]", who);
    if (r[3] < 0 || r[3] > 1) return fail(HK_E_INVALID, "%s: aux done not 0 or 1", who);
    if (r[4] < -1 || r[4] > 1) return fail(HK_E_INVALID, "%s: aux winner not -1, 0 or 1", who);
  }
  return HK_OK;
}

int hk_reset(void *ctx, const uint8_t *mask, const float *params, const int32_t *max_t, const uint8_t *one_starts,
             void *stream) {
  HK_ENTER(ctx, "hk_reset");
  if (max_t) {
    const int rc = check_ints("hk_reset", c->s.n, 1, max_t, mask, (hipStream_t)stream);
    if (rc != HK_OK) return rc;
  }
  return launched(hk::launch_reset(c->s, c->cfg, mask, params, max_t, one_starts, (hipStream_t)stream), "hk_reset");
}

int hk_seeded_params(void *ctx, const uint64_t *seeds, const uint8_t *one_starts, float *params, int32_t *max_t,
                     void *stream) {
  HK_CTX(ctx, "hk_seeded_params");
  if (!seeds || !params) return fail(HK_E_INVALID, "hk_seeded_params: NULL argument%s");
  HK_QUIESCED(c, "hk_seeded_params");
  return launched(hk::launch_seeded_params(c->s, c->cfg, nullptr, seeds, one_starts, 0, params, max_t, nullptr,
                                           (hipStream_t)stream),
                  "hk_seeded_params");
}

// Two launches on `stream`: the placement kernel (hk_seeded_reset.hip) into the context's scratch, then hk_reset's
// own kernel with that scratch as its explicit params and puck sides -- the reset itself stays single source.
int hk_reset_seeded(void *ctx, const uint8_t *mask, const uint64_t *seeds, const int32_t *max_t,
                    const uint8_t *one_starts, void *stream) {
  HK_CTX(ctx, "hk_reset_seeded");
  if (!seeds) return fail(HK_E_INVALID, "hk_reset_seeded: seeds is NULL%s");
  HK_QUIESCED(c, "hk_reset_seeded");
  if (max_t) {
    const int rc = check_ints("hk_reset_seeded", c->s.n, 1, max_t, mask, (hipStream_t)stream);
    if (rc != HK_OK) return rc;
  }
  const hipError_t e = hk::launch_seeded_params(c->s, c->cfg, mask, seeds, one_starts, 1, c->seed_params, nullptr,
                                                c->seed_one, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "hk_reset_seeded");
  return launched(hk::launch_reset(c->s, c->cfg, mask, c->seed_params, max_t, c->seed_one, (hipStream_t)stream),
                  "hk_reset_seeded");
}

static int launch_steps(const char *who, void *ctx, const hk_step_io *io, int nsteps, void *stream) {
  HK_CTX(ctx, who);
  if (!io) return fail(HK_E_INVALID, "%s: NULL argument", who);
  if (nsteps < 1) return fail(HK_E_INVALID, "%s: n_steps must be >= 1", who);
  if (!io->actions && (c->cfg.policy[0] == HK_POLICY_EXTERNAL || c->cfg.policy[1] == HK_POLICY_EXTERNAL))
    return fail(HK_E_INVALID, "%s: a player takes external actions but io->actions is NULL", who);
  if (io->policy2 && !io->actions)  // an override may pick HK_POLICY_EXTERNAL for any arena
    return fail(HK_E_INVALID, "%s: io->policy2 is given but io->actions is NULL", who);
  hk::StepIO s{};
  s.actions = io->actions;
  s.opp_inc = io->opp_inc;
  s.obs = io->obs;
  s.obs2 = io->obs2;
  s.reward = io->reward;
  s.reward2 = io->reward2;
  s.done = io->done;
  s.info = io->info;
  s.info2 = io->info2;
  s.actions_out = io->actions_out;
  s.debug = io->debug;
  s.final_obs = io->final_obs;
  s.flags = io->flags;
  s.policy2 = io->policy2;
  s.record = io->record;
  HK_QUIESCED(c, who);
  return launched(hk::launch_step(c->s, c->cfg, s, nsteps, (hipStream_t)stream), who);
}

int hk_step(void *ctx, const hk_step_io *io, void *stream) { return launch_steps("hk_step", ctx, io, 1, stream); }

int hk_step_host(void *ctx, const float *actions, const double *opp_inc, int32_t flags, void *out, void *stream) {
  if (!ctx || !out) return fail(HK_E_INVALID, "hk_step_host: NULL argument%s");
  Ctx *c = (Ctx *)ctx;
  if (c->s.n != 1) return fail(HK_E_INVALID, "hk_step_host: only single-arena contexts (n_arenas == 1)%s");
  if (!actions && (c->cfg.policy[0] == HK_POLICY_EXTERNAL || c->cfg.policy[1] == HK_POLICY_EXTERNAL))
    return fail(HK_E_INVALID, "hk_step_host: a player takes external actions but actions is NULL%s");
  DeviceGuard g(c->device);
  return c->hs.step(c->s, c->cfg, {actions, opp_inc, flags, out, (hipStream_t)stream});
}

int hk_rollout(void *ctx, int32_t n_steps, const hk_step_io *io, void *stream) {
  return launch_steps("hk_rollout", ctx, io, n_steps, stream);
}

int hk_get_state(void *ctx, float *state, int32_t *aux, void *stream) {
  HK_ENTER(ctx, "hk_get_state");
  return launched(hk::launch_get_state(c->s, c->cfg, state, aux, (hipStream_t)stream), "hk_get_state");
}

int hk_set_state(void *ctx, const uint8_t *mask, const float *state, const int32_t *aux, void *stream) {
  HK_ENTER(ctx, "hk_set_state");
  if (aux) {
    const int rc = check_ints("hk_set_state", c->s.n, 5, aux, mask, (hipStream_t)stream);
    if (rc != HK_OK) return rc;
  }
  return launched(hk::launch_set_state(c->s, c->cfg, mask, state, aux, (hipStream_t)stream), "hk_set_state");
}

int hk_observe(void *ctx, float *obs, float *obs2, void *stream) {
  HK_ENTER(ctx, "hk_observe");
  return launched(hk::launch_observe(c->s, c->cfg, obs, obs2, (hipStream_t)stream), "hk_observe");
}

int hk_info(void *ctx, double *info, double *info2, double *reward, double *reward2, void *stream) {
  HK_ENTER(ctx, "hk_info");
  return launched(hk::launch_info(c->s, c->cfg, info, info2, reward, reward2, (hipStream_t)stream), "hk_info");
}

int hk_opponent_phase(void *ctx, double *phase_out, const double *phase_in, void *stream) {
  return phase_rows("hk_opponent_phase", ctx, 2, phase_out, phase_in, stream);
}

int hk_opponent_phase3(void *ctx, double *phase_out, const double *phase_in, void *stream) {
  return phase_rows("hk_opponent_phase3", ctx, 3, phase_out, phase_in, stream);
}

// ---- exact arena snapshots, restore and fork (hk_arena_copy.h) ----
static_assert(HK_CNT_BAD_INDEX < HK_NUM_COUNTERS, "the bad-index word is one of the context's counters");

int64_t hk_snapshot_bytes(int64_t m) { return m < 0 ? 0 : hk::blob_layout(m).bytes; }

int hk_snapshot_layout(int32_t *out5) {
  if (!out5) return fail(HK_E_INVALID, "hk_snapshot_layout: NULL argument%s");
  out5[0] = hk::NFF;
  out5[1] = hk::NPW;
  out5[2] = hk::kPhaseRows;
  out5[3] = hk::NSOLID;
  out5[4] = hk::NMF;
  return HK_OK;
}

static int check_blob(const char *who, const void *blob, int64_t m) {
  if (m < 0) return fail(HK_E_INVALID, "%s: negative count %lld", who, m);
  if (m > 0 && !blob) return fail(HK_E_INVALID, "%s: blob is NULL", who);
  if ((uintptr_t)blob & 15) return fail(HK_E_INVALID, "%s: blob is not 16-byte aligned", who);
  return HK_OK;
}

int hk_snapshot(void *ctx, const int64_t *idx, int64_t m, void *blob, void *stream) {
  HK_CTX(ctx, "hk_snapshot");
  if (const int rc = check_blob("hk_snapshot", blob, m)) return rc;
  HK_QUIESCED(c, "hk_snapshot");
  return launched(hk::launch_copy_arenas(hk::blob_view(blob, m), nullptr, hk::view_of(c->s), idx, m,
                                         c->s.counters + HK_CNT_BAD_INDEX, (hipStream_t)stream),
                  "hk_snapshot");
}

int hk_restore(void *ctx, const int64_t *idx, int64_t m, const void *blob, int64_t blob_m, const int64_t *rows,
               void *stream) {
  HK_CTX(ctx, "hk_restore");
  if (const int rc = check_blob("hk_restore", blob, m)) return rc;
  if (blob_m < 0 || (m > 0 && blob_m == 0)) return fail(HK_E_INVALID, "hk_restore: bad blob_m %s%lld", "", blob_m);
  HK_QUIESCED(c, "hk_restore");
  return launched(hk::launch_copy_arenas(hk::view_of(c->s), idx, hk::blob_view(const_cast<void *>(blob), blob_m), rows,
                                         m, c->s.counters + HK_CNT_BAD_INDEX, (hipStream_t)stream),
                  "hk_restore");
}

int hk_copy_arenas(void *dst_ctx, const int64_t *dst_idx, void *src_ctx, const int64_t *src_idx, int64_t m,
                   void *stream) {
  if (!dst_ctx || !src_ctx) return fail(HK_E_INVALID, "hk_copy_arenas: ctx is NULL%s");
  Ctx *d = (Ctx *)dst_ctx, *s = (Ctx *)src_ctx;
  if (m < 0) return fail(HK_E_INVALID, "hk_copy_arenas: negative count %s%lld", "", m);
  if (d->device != s->device) return fail(HK_E_INVALID, "hk_copy_arenas: the contexts are on different devices%s");
  if (d->cfg.keep_mode != s->cfg.keep_mode || d->cfg.vel_ref != s->cfg.vel_ref)
    return fail(HK_E_INVALID, "hk_copy_arenas: the contexts differ in keep_mode or vel_ref_semantics%s");
  DeviceGuard g(d->device);
  if (const int q = d->hs.quiesce("hk_copy_arenas")) return q;
  if (s != d)
    if (const int q = s->hs.quiesce("hk_copy_arenas")) return q;
  return launched(hk::launch_copy_arenas(hk::view_of(d->s), dst_idx, hk::view_of(s->s), src_idx, m,
                                         d->s.counters + HK_CNT_BAD_INDEX, (hipStream_t)stream),
                  "hk_copy_arenas");
}

int hk_counters(void *ctx, int64_t *out, void *stream) {
  HK_CTX(ctx, "hk_counters");
  if (!out) return fail(HK_E_INVALID, "hk_counters: NULL argument%s");
  HK_QUIESCED(c, "hk_counters");
  hipError_t e = hipMemcpyAsync(out, c->s.counters, HK_NUM_COUNTERS * 8, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  return launched(e, "hk_counters");
}

int hk_reset_counters(void *ctx, void *stream) {
  HK_ENTER(ctx, "hk_reset_counters");
  return launched(hipMemsetAsync(c->s.counters, 0, HK_NUM_COUNTERS * 8, (hipStream_t)stream), "hk_reset_counters");
}

int hk_bytes_per_step(const void *ctx, int64_t *algorithmic, int64_t *implementation) {
  if (!ctx) return fail(HK_E_INVALID, "hk_bytes_per_step: ctx is NULL%s");
  // action 32 B + body state 72 B + 4 int32 scalars 16 B read; body state 72 B,
  // scalars 16 B, obs 72 B, reward 4 B, done 1 B written = 285 B per env-step.
  if (algorithmic) *algorithmic = 285;
  // implementation (excluding manifolds, which are only touched where a pair is in contact):
  // f: 29 floats read+write, i: 6 packed int words read+write (r06; 12 before), obs 72 + reward 4 + done 1 + info 16.
  if (implementation) *implementation = (int64_t)(hk::NFF * 4 * 2 + hk::NPW * 4 * 2 + 72 + 4 + 1 + 16);
  return HK_OK;
}

}  // extern "C"

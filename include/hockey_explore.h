/* hockey_explore.h -- exploration acting of the learner library (libhockey_learner.so): included by hockey_learner.h,
 * which defines hkl_act_io, HKL_GROUP_MAX and the error codes this header uses; include that one. */
#ifndef HOCKEY_EXPLORE_H
#define HOCKEY_EXPLORE_H
#ifndef HOCKEY_LEARNER_H
#error "include hockey_learner.h"
#endif

/* ---- exploration acting (hockey_amd/explore.py; csrc/hkl_explore.h) ----
 * hkl_act with TD3.act's exploration (rl/td3/agent.py get_action, _update_noise_scale) as the acting kernel's
 * epilogue, for S = n_rows / rows_per_member members side by side: member m owns rows [m n, (m + 1) n), n =
 * rows_per_member, and local(i) = i - m n is a row's index inside its member.  `act` is hkl_act's struct with hkl_act's
 * contract (K <= 64; policy == NULL runs slot 0 on every row; a row whose policy lies outside [0, K) is not written).
 * For an acting row i of member m, with a = hkl_act's action of the row (the same bits):
 *
 *   T0 = max(total[m], 0), T1 = T0 + min(max(count[m], 0), n)
 *   all_random(m) = T1 < start_steps;   random(i) = all_random(m) || T0 + 1 + local(i) < start_steps
 *   progress = min((double)T1 / (double)max_total_steps, 1.0)
 *   scale    = init_scale                                        anneal NONE, or max_total_steps <= 0
 *              max(init_scale * (1 - progress), min_scale)       LINEAR
 *              max(init_scale * pow(0.1, progress), min_scale)   EXP          -- float64, then s_m = (float)scale
 *   out[i][c] = random(i) ? 2 u - 1                      u = (w_c >> 8) 2^-24 of the row's random-phase block
 *                         : clamp(fadd(a, fmul(unit, s_m)), -1, 1)            two roundings, NaN stays NaN
 *
 * Draws are Philox4x32-10 blocks, key = seed_m ^ purpose, counter = (local lo, local hi, calls[m] lo, calls[m] hi):
 * a function of the member's seed, the row's index inside the member and the member's call counter, never of the
 * row's position in the batch or in the grouping.  HKL_EXPLORE_KEY_NOISE is the noise block, HKL_EXPLORE_KEY_RANDOM
 * the random-phase block; component c takes word c.  unit per noise mode:
 *   NONE      0
 *   GAUSSIAN  z_c: the four Box-Muller normals of the noise block (hkl_sample's construction)
 *   UNIFORM   (2 u_c - 1) * (float)sqrt(3)
 *   OU        x' = fadd(fadd(x, fmul(fmul(theta, -x), dt)), fmul(sqrt_dt, z_c)), x = x[i][c]; unit = x', and x[i][c] :=
 *             x' -- an Ornstein-Uhlenbeck process of sigma 1 (it is linear in sigma from x = 0, so the product with
 *             s_m is the reference's noise * (current / initial)).  The state advances in every call in which the
 *             member is not all_random, for every acting row of the member, random(i) or not, as TD3.act's does.
 *   EXTERNAL  ext[i * ext_ld + c * ext_cs]: the caller's noise of unit scale (pink blocks)
 * A member that is all_random draws no noise and leaves x alone.
 *
 * Optional outputs: z_out [n_rows][4] receives for every acting row the raw noise draw computed for it (the normals;
 * UNIFORM: 2 u - 1; 0 where none was computed: NONE, EXTERNAL, an all_random member); scale_out [S] receives s_m.
 * After the acting kernel a one-workgroup kernel stores total[m] = T1 and calls[m] += 1 (and scale_out); the acting
 * workgroups only read the state.  count[m] is the caller's: the member's arenas still running (n without early
 * episode ends).  Negative total / count and count > n are clamped as above and nothing read from the device is used
 * as an index.  A non-finite observation row gives non-finite actions (and OU state) in that row alone.
 *
 * members_host is the caller's host copy of the S structs, io->members the same bytes in device memory (uploaded once
 * per run).  Asynchronous on stream, graph-capturable, nothing read back; kernel launches only (two without policy,
 * six with: the counters are zeroed by a kernel, hkl_act's three grouping kernels follow), so a capture is a line of
 * kernel nodes.  HKL_E_INVALID:
 * hkl_act's faults, n_rows == 0, rows_per_member <= 0, n_rows not a multiple of rows_per_member, S outside
 * [1, HKL_GROUP_MAX], a null members / members_host / total / calls / count, an anneal or noise id out of range, a
 * null x with an OU member, a null ext with an EXTERNAL member. */
#define HKL_EXPLORE_KEY_NOISE 0x6578706C6F7265ull /* "explore" */
#define HKL_EXPLORE_KEY_RANDOM 0x72616E646F6Dull  /* "random" */
enum { HKL_ANNEAL_NONE = 0, HKL_ANNEAL_LINEAR = 1, HKL_ANNEAL_EXP = 2 };
enum { HKL_NOISE_NONE = 0, HKL_NOISE_GAUSSIAN = 1, HKL_NOISE_UNIFORM = 2, HKL_NOISE_OU = 3, HKL_NOISE_EXTERNAL = 4 };
typedef struct {
  uint64_t seed;
  int64_t start_steps, max_total_steps; /* max_total_steps 0: no schedule, the scale stays init_scale */
  double init_scale, min_scale;
  int32_t anneal, noise;
  float theta, dt, sqrt_dt; /* OU */
  int32_t reserved;
} hkl_explore_member;
typedef struct {
  hkl_act_io act;
  int32_t rows_per_member;
  const hkl_explore_member *members; /* device [S] */
  int64_t *total, *calls;            /* device [S] */
  const int32_t *count;              /* device [S] */
  float *x;                          /* device [n_rows][4]: OU state */
  const float *ext;                  /* EXTERNAL members' unit noise */
  int64_t ext_ld, ext_cs;
  float *z_out, *scale_out;
} hkl_explore_io;
int hkl_explore_io_size(void);
int hkl_explore_member_size(void);
int hkl_explore(const hkl_explore_io *io, const hkl_explore_member *members_host, void *stream);

#endif

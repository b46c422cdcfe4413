/* hockey_learner.h -- C ABI of the fused fp32 MFMA TD3 learner (libhockey_learner.so, gfx950).
 *
 * Replaces, for large learner batches, the PyTorch ops of one rl/td3/learner.py TD3Learner.update
 * (:55-72): compute_target (:75-112), update_critic (:115-136), update_actor (:138-175) and soft_update (:196-218),
 * with Adam (rl/td3/agent.py:174-182).  hockey_amd/learner_hip.py binds it with ctypes; every pointer is a device
 * pointer (torch tensors' storage), every call is asynchronous on `stream` (a hipStream_t) and graph-capturable.
 * Batches are multiples of 256.  Returns HKL_OK or an error code; hkl_last_error() describes the last failure: after
 * every call that returns non-zero it reads "<entry point>: <what is wrong>".  A refused call (HKL_E_INVALID) has
 * launched nothing.
 */
#ifndef HOCKEY_LEARNER_H
#define HOCKEY_LEARNER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HKL_OK 0
#define HKL_E_INVALID 1
#define HKL_E_DEVICE 2
#define HKL_MAX_SEG 12
/* floats of one network's MFMA operand pack (csrc/hkl_mlp.h: f1, fp, bp, fo, wa) */
#define HKL_PACK_FLOATS (16 * 64 * 8 + 2 * 16 * 16 * 64 * 4 + 16 * 64 * 4 + 256 * 4)

/* one MLP n_in -> 256 -> 256 -> n_out (tanh hidden; rl/td3/networks.py ActorNetwork): torch Linear weights
 * [out][in] row-major, and its operand pack (hkl_pack writes it from the weights) */
typedef struct {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  float *pack;
  int32_t n_in, n_out;
} hkl_net;

/* compute_target + update_critic forward / backward for both critics.  Inputs: the replay ring's columns
 * (s [cap][18], a [cap][4], r [cap], s2 [cap][18], d [cap]), the sampled slots idx [B], the clipped target noise
 * [B][4], optional importance weights iw [B].  Outputs: X0 [B][32] (critic inputs), per critic k: H1, DZ1, DZ2
 * [B][256]; workgroup partials (B / 64 rows) of db1, db2, dW3 [.][256] and db3 [.]; loss partials [B / 64];
 * optional td [B] = (|q1 - y| + |q2 - y|) / 2 for prioritized replay.  (db1 / db2 come from hkl_wgrad's
 * column sums; p_db1 / p_db2 are unused.) */
typedef struct {
  int64_t batch;
  const int64_t *idx;
  const float *ring_s, *ring_a, *ring_r, *ring_s2, *ring_d;
  const float *noise, *iw;
  hkl_net target_actor, target_q[2], q[2];
  float gamma;
  float act_low[4], act_range[4];
  float *x0, *h1[2], *dz1[2], *dz2[2];
  float *p_db1[2], *p_db2[2], *p_dw3[2], *p_db3[2];
  float *p_loss, *td;
  int64_t *sample_counter; /* optional: hkl_sample's update counter, advanced by one at the end */
} hkl_critic_io;

/* update_actor forward / backward: actor(s), Q1(s, actor(s)) of the updated critic, d(-mean Q1).  Outputs: X0
 * [B][32], H1, H2, DZ1, DZ2 [B][256]; workgroup partials of dW3 [.][4][256], db3 [.][4]; loss partials
 * (p_db1 / p_db2 unused). */
typedef struct {
  int64_t batch;
  const int64_t *idx;
  const float *ring_s;
  hkl_net actor, q1;
  float act_low[4], act_range[4];
  float *x0, *h1, *h2, *dz1, *dz2;
  float *p_db1, *p_db2, *p_dw3, *p_db3;
  float *p_loss;
} hkl_actor_io;

/* one parameter tensor for hkl_adam: grad[r][c] = sum_{k < chunks} src[k * stride + r * ld + c]; target
 * (optional): the tensor's soft-update twin in the target network, updated when hkl_adam_io.polyak is set */
typedef struct {
  float *param, *m, *v;
  const float *src;
  int32_t rows, cols;
  int64_t ld;
  int32_t chunks;
  int64_t stride;
  float *target;
} hkl_seg;

typedef struct {
  hkl_seg seg[HKL_MAX_SEG];
  int32_t n_seg;
  float lr;
  double beta1, beta2; /* double: the kernel rounds 1 - beta from it, as torch does from its Python scalars */
  float eps, wd;
  const int64_t *step;           /* optimiser steps taken so far (device); hkl_pack advances it */
  const float *loss_src;         /* optional: loss partials; *loss_sum += their sum x loss_scale, *loss_count += 1 */
  int32_t loss_chunks;
  float loss_scale;
  double *loss_sum, *loss_count;
  /* polyak != 0: after its Adam step every parameter p with a segment target t also takes soft_update
   * (learner.py:214-218): t = t * polyak_rho + polyak_tau * p, each product rounded (torch's mul_ then add_) --
   * the same values as hkl_polyak after hkl_adam, one launch fewer */
  int32_t polyak;
  float polyak_rho, polyak_tau;
} hkl_adam_io;

typedef struct {
  hkl_net net[4];
  int64_t *step;
} hkl_pack_io;

const char *hkl_last_error(void);
int hkl_pack_floats(void);
/* re-lay the weights of 1..4 networks out as MFMA operands; advances *step by one when step != NULL.  Refused: a null
 * nets, or a network with a null weight, bias or pack pointer (as hkl_pack_group refuses it). */
int hkl_pack(const hkl_net *nets, int n_nets, int64_t *step, void *stream);
/* Both refuse what their grouped forms refuse in a member: a batch that is no positive multiple of 256 and a null in
 * any pointer the kernel dereferences unconditionally (every one but iw, td, sample_counter, p_db1 and p_db2). */
int hkl_critic_step(const hkl_critic_io *io, void *stream);
int hkl_actor_step(const hkl_actor_io *io, void *stream);
/* weight-gradient job: slab[c][256][k_width] = sum over the samples j of chunk c (k_width 256: 512 samples each
 * when the launch has two or more k-width-256 jobs and the batch is a multiple of 512, else 256; k_width 32: 256)
 * of dz[j][o] x[j][k]
 * (dz [B][256], x [B][k_width]); bias_slab (optional) [c][256] = the chunk's column sums of dz */
typedef struct {
  const float *dz, *x;
  float *slab, *bias_slab;
} hkl_wgrad_job;
/* 1..4 jobs of one k_width (256 or 32) in one launch.  A job with a null dz, x or slab is refused here and in
 * hkl_wgrad_pair, as in hkl_wgrad_pair_group (bias_slab stays optional). */
int hkl_wgrad(const hkl_wgrad_job *jobs, int n_jobs, int k_width, int64_t batch, void *stream);
/* hkl_wgrad for n_wide k-width-256 jobs (dW2) and n_narrow k-width-32 jobs (dW1) in one launch (the same slabs as
 * the two hkl_wgrad calls, bit for bit). */
int hkl_wgrad_pair(const hkl_wgrad_job *wide, int n_wide, const hkl_wgrad_job *narrow, int n_narrow, int64_t batch,
                   void *stream);
/* Refused: n_seg outside [1, HKL_MAX_SEG], a null step, a segment with a null param / m / v / src (or target with
 * polyak set), loss_src without loss_sum and loss_count -- the checks of hkl_adam_group on a member. */
int hkl_adam(const hkl_adam_io *io, void *stream);
/* target = target * rho + tau * param over n floats (soft_update; tau = 1 - rho) */
int hkl_polyak(float *target, const float *param, int64_t n, float rho, float tau, void *stream);

/* the batch's replay slots idx[B] (uniform over the ring's *size filled slots) and clipped target noise [B][4]
 * from Philox4x32-10 keyed by seed, counter = *counter (device; hkl_critic_step advances it) */
typedef struct {
  int64_t batch;
  uint64_t seed;
  const int64_t *counter, *size;
  int64_t *idx;
  float *noise;
  float scale, clip;
} hkl_sample_io;
/* Any batch >= 1 (hkl_sample_group: a multiple of 256); counter, size, idx and noise must not be null. */
int hkl_sample(const hkl_sample_io *io, void *stream);

/* ---- grouped forms: n_members <= HKL_GROUP_MAX independent learners in the launch one learner takes
 * (hockey_amd/population.py).  Member m runs in its own slice of the grid (blockIdx.y; blockIdx.z for pack) and reads
 * its struct from an array in device memory: 64 x sizeof(hkl_critic_io) is far beyond the kernel-argument segment.
 *
 *  - host: the caller's host copy of the n_members structs.  Every check of the single call runs on it for every
 *    member; in addition n_members must lie in [1, HKL_GROUP_MAX], dev must not be null, the members' batch must be
 *    equal (a positive multiple of 256, hkl_sample_group included), every pointer the kernel dereferences
 *    unconditionally must be non-null (the optional ones stay optional: iw, td, sample_counter, bias_slab, loss_src,
 *    pack's step), and for hkl_adam_group n_seg and every segment's rows x cols must be equal across members (chunks,
 *    ld, stride, lr, wd, betas, polyak may differ).  A failed check returns HKL_E_INVALID, hkl_last_error names the
 *    call, the member and what is wrong, and nothing is launched.
 *  - dev: the same bytes in device memory, uploaded by the caller once.  That the two agree, and that the members'
 *    output buffers are disjoint, is the caller's contract.
 *  - One launch per call; asynchronous on stream, graph-capturable, no host synchronisation and no copy in the call.
 *  - Member m's results are bit for bit those of the single call on host[m], whatever the other members are: the
 *    same kernel body runs on the same grid slice.
 *  - hkl_wgrad_pair_group: the arrays are [n_members][n_wide] and [n_members][n_narrow]; chunking as hkl_wgrad_pair
 *    at the same n_wide / n_narrow / batch.  hkl_pack_group packs net[0 .. n_nets) of every member.
 *  - hkl_adam_io.polyak is part of the struct: a caller that alternates it (the critic's Adam on critic-only and on
 *    critic + actor updates) keeps two device arrays.
 * Prioritized replay has grouped forms of its own under the same contract: hkl_per_*_group, after the hkl_per_* calls
 * below. */
#define HKL_GROUP_MAX 64
int hkl_sample_group(const hkl_sample_io *host, const hkl_sample_io *dev, int n_members, void *stream);
int hkl_critic_step_group(const hkl_critic_io *host, const hkl_critic_io *dev, int n_members, void *stream);
int hkl_actor_step_group(const hkl_actor_io *host, const hkl_actor_io *dev, int n_members, void *stream);
int hkl_wgrad_pair_group(const hkl_wgrad_job *wide_host, const hkl_wgrad_job *wide_dev, int n_wide,
                         const hkl_wgrad_job *narrow_host, const hkl_wgrad_job *narrow_dev, int n_narrow, int64_t batch,
                         int n_members, void *stream);
int hkl_adam_group(const hkl_adam_io *host, const hkl_adam_io *dev, int n_members, void *stream);
int hkl_pack_group(const hkl_pack_io *host, const hkl_pack_io *dev, int n_nets, int n_members, void *stream);

/* ---- prioritized replay (rl/replay/prioritized_buffer.py) on per-block sums: csrc/hkl_per.h ----
 * Slot i of the ring has the sanitised weight p_i = max(nan_to_num(w_i, 0, 0, 0), 1e-6f) for i < *size and 0
 * otherwise; every sum of them is taken in float64 in a fixed order.  The ring's slots are cut into blocks of
 * HKL_PER_BLOCK; bsum / bmax hold each block's sum of p and its maximum raw weight (NaN propagates, as torch's max),
 * so that sampling, the priority write-back and a push touch only the blocks they need. */
#define HKL_PER_BLOCK 1024
/* with nblk = ceil(cap / HKL_PER_BLOCK): */
typedef struct {
  int64_t cap;
  float *w;            /* [cap] the ring's raw weights */
  const int64_t *size; /* the ring's fill level */
  double *bsum;        /* [nblk] */
  float *bmax;         /* [nblk] */
  double *bpre;        /* [nblk] scratch: inclusive prefix of bsum (hkl_per_sample rewrites it) */
  int32_t *last;       /* [cap] scratch, all zero between calls: hkl_per_update's last position + 1 of a slot */
  int32_t *bown;       /* [nblk] scratch, all zero between calls: the position + 1 that refreshes a touched block */
} hkl_per;

/* idx[e] = the first slot whose inclusive CDF of p exceeds u_e * sum(p) (searchsorted(..., right=True)), clamped to
 * *size - 1; u_e = u[e] when u is given, else hkl_sample's 53-bit Philox draw for (seed, e, *counter).  noise
 * (optional) [B][4]: hkl_sample's clipped target noise for the same (seed, e, *counter), bit for bit.  iw (optional)
 * [B]: the importance weights (1 / (p_b * *size)) ** beta / their maximum, p_b = w[idx] / sum_batch(w[idx]) on the
 * raw weights (learner.py:199-210).  Any batch >= 1. */
typedef struct {
  hkl_per per;
  int64_t batch;
  uint64_t seed;
  const int64_t *counter; /* required when u is NULL; hkl_critic_step advances it */
  const double *u;
  int64_t *idx;
  float *noise;
  float scale, clip;
  float *iw;
  double beta;
} hkl_per_sample_io;

/* w[idx[e]] = clamp(td[e], 1e-6, 1e6); of a slot that occurs more than once the last occurrence wins (numpy's
 * fancy assignment, prioritized_buffer.py:67-69); then bsum / bmax of every touched block are recomputed */
typedef struct {
  hkl_per per;
  int64_t batch;
  const int64_t *idx;
  const float *td;
} hkl_per_update_io;

int hkl_per_block(void);
/* recompute bsum / bmax of the blocks that cover slots [lo, lo + n); n == cap rebuilds everything */
int hkl_per_refresh(const hkl_per *per, int64_t lo, int64_t n, void *stream);
/* PrioritizedRing._before_push: slots pos .. pos + n - 1 (wrapping) get max(w[0 : size_after]) of the weights
 * before the call; their blocks are recomputed against the fill level size_after (the caller stores it to *size) */
int hkl_per_push(const hkl_per *per, int64_t pos, int64_t n, int64_t size_after, void *stream);
int hkl_per_sample(const hkl_per_sample_io *io, void *stream);
/* hkl_per_sample's importance weights alone, for the slots already in io->idx */
int hkl_per_weights(const hkl_per_sample_io *io, void *stream);
int hkl_per_update(const hkl_per_update_io *io, void *stream);

/* ---- grouped prioritized replay: the hkl_per_* calls for n_members <= HKL_GROUP_MAX rings at once
 * (hockey_amd/population.py PopulationPrioritizedRing), under the grouped forms' contract above: host is checked in
 * full (every check of the single call, on every member) before anything is launched, dev holds the same bytes on the
 * device, member m runs in grid slice blockIdx.y, and a failed check returns HKL_E_INVALID with the call, the member
 * and the fault in hkl_last_error.  Every call is asynchronous on stream and graph-capturable, with no host
 * synchronisation, no copy and no read-back, and its number of launches depends neither on n_members nor on any
 * value held on the device.  Member m's results are bit for bit those of the single call on host[m], whatever the
 * other members are: the kernels share the single kernels' bodies, and with them every fixed summation order (a
 * block's slot-by-slot and lane-by-lane sums, the prefix scan, the importance weights' tree).
 *
 *  - In every call the members' cap must be equal (one block count, one grid), in the sample / weights / update calls
 *    their batch too (any batch >= 1, as in the single calls), and every member's w must be 16-byte aligned (a block
 *    is read as float4; a ring that is a slice of a larger storage is placed accordingly).
 *  - The members' w, bsum, bmax, bpre, last and bown must be pairwise disjoint: that is the caller's contract.
 *  - hkl_per_sample_group: prefix, draw and importance weights, three launches.  Per member u or counter must be
 *    non-null; noise, iw, beta, seed, scale and clip are per member, noise and iw optional per member (a member
 *    without iw takes no weights).  hkl_per_weights_group: the importance weights alone for the slots already in idx
 *    (iw required), one launch.  hkl_per_update_group: mark, write and touch, three launches.
 *  - hkl_per_refresh_group recomputes every block of every member against its *size: one launch.
 *  - hkl_per_push_group: pos, n and size_after are DEVICE arrays int64[n_members].  A member with n[m] > 0 gets
 *    exactly hkl_per_push(&host[m], pos[m], n[m], size_after[m]): the maximum of w[0 : size_after) before the call is
 *    stored to the n pushed slots, wrapping, and the covered blocks are recomputed against size_after (the caller
 *    stores it to *size, before or after the call).  A member with n[m] == 0 is untouched.  max_n is the host's upper
 *    bound on every n[m], 1 <= max_n <= cap: it sizes the grid, which covers the blocks a push of max_n slots can
 *    touch (head and wrapped tail); waves with nothing to do exit.  Two launches.  0 <= n[m] <= max_n, 0 <= pos[m] <
 *    cap and n[m] <= size_after[m] <= cap are the caller's contract, which the host cannot check; the kernels cut a
 *    count to max_n and a fill level to cap and skip a member whose pos lies outside the ring, so values outside the
 *    contract never address memory outside the member's arrays. */
int hkl_per_sample_group(const hkl_per_sample_io *host, const hkl_per_sample_io *dev, int n_members, void *stream);
int hkl_per_weights_group(const hkl_per_sample_io *host, const hkl_per_sample_io *dev, int n_members, void *stream);
int hkl_per_update_group(const hkl_per_update_io *host, const hkl_per_update_io *dev, int n_members, void *stream);
int hkl_per_refresh_group(const hkl_per *host, const hkl_per *dev, int n_members, void *stream);
int hkl_per_push_group(const hkl_per *host, const hkl_per *dev, const int64_t *pos, const int64_t *n,
                       const int64_t *size_after, int64_t max_n, int n_members, void *stream);

/* y = the kernels' tanh of x (n floats; a test probe of the activation's accuracy) */
int hkl_tanh_probe(const float *x, float *y, int64_t n, void *stream);

/* ---- actor inference over a bank of policies (hockey_amd/policy_bank.py) ----
 * A bank is n_policies <= HKL_ACT_MAX_POLICIES actors 18 -> 256 -> 256 -> 4 (tanh hidden and output) in two strided
 * buffers: params [K][HKL_ACT_PARAM_FLOATS] = fc1.weight [256][18], fc1.bias, fc2.weight [256][256], fc2.bias,
 * fc3.weight [4][256], fc3.bias of each slot in torch layout, and packs [K][HKL_PACK_FLOATS], slot k written by
 * hkl_pack from a hkl_net that points into params[k] (n_in 18, n_out 4).
 *
 * Row i < n_rows with policy[i] = k in [0, K): out[i * out_ld + out_col .. + 4) = slot k's actor on obs[i * obs_ld ..
 * + 18).  A row with policy[i] = -1 (or any id outside [0, K)) is not written, and no other float of out is.
 * policy == NULL: every row runs slot 0 and nothing is grouped (order / counts / offsets may be NULL).  With policy
 * given the rows are grouped by policy on the device in the caller's scratch: order [n_rows], counts and offsets
 * [HKL_ACT_MAX_POLICIES + 1] each (int32; contents on entry irrelevant, overwritten).  A row's result does not depend
 * on the other rows, their policies or its position (bit for bit).  Asynchronous on stream, graph-capturable, no
 * host synchronisation.  HKL_E_INVALID: K outside [1, 64], n_rows < 0, obs_ld < 18, out_col < 0, out_ld < out_col + 4,
 * a null params / packs / obs / out, or null scratch with policy given. */
#define HKL_ACT_MAX_POLICIES 64
#define HKL_ACT_PARAM_FLOATS (256 * 18 + 256 + 256 * 256 + 256 + 4 * 256 + 4)
typedef struct {
  int32_t n_policies, n_rows;
  const float *params, *packs;
  const float *obs;
  int64_t obs_ld;
  const int32_t *policy;
  float *out;
  int64_t out_ld;
  int32_t out_col;
  int32_t *order, *counts, *offsets;
} hkl_act_io;
int hkl_act_io_size(void);
int hkl_act(const hkl_act_io *io, void *stream);

/* ---- exploration acting: hkl_explore, hkl_act with TD3.act's exploration as the acting kernel's epilogue.  Its
 * contract, structs and declaration fill a header of their own, which builds on hkl_act_io and HKL_GROUP_MAX above. */
#include "hockey_explore.h"

/* ---- collection on the device: the opponent draw before the step and the replay store after it, in a header of
 * their own beside the exploration's. */
#include "hockey_collect.h"

/* ---- evaluation on the device: the accounting of the evaluation loop for many cells side by side and its fold, in a
 * header of their own beside the collection's. */
#include "hockey_eval.h"

/* ---- actor inference over a wide bank (population self-play: one pool of snapshots per member) ----
 * hkl_act's contract with K = n_policies in [1, HKL_ACT_WIDE_MAX_POLICIES]: params, packs, obs, policy and out as
 * above, a row with policy[i] outside [0, K) is not written, no other float of out is, and a row's four actions are
 * hkl_act's bit for bit (both acting kernels run one body).  policy == NULL: every row runs slot 0, no scratch.
 * With policy given the caller provides the scratch (int32; contents on entry irrelevant, overwritten):
 *   order   [n_rows]          the acting rows, grouped by policy
 *   counts  [K + 1]           rows per policy (then the scatter's cursors); counts[K] = the number of tiles
 *   offsets [K + 1]           exclusive scan of the counts
 *   tiles   [3 * max_tiles]   (policy, first position in order, rows left in the group) of each 64-row tile,
 *                             max_tiles = min(n_rows, (n_rows + 63) / 64 + K): a bound on the non-empty tiles
 * Five launches whatever K and the device values are; the acting grid is max_tiles workgroups and the
 * surplus ones leave at once.  Asynchronous on stream, graph-capturable, no host synchronisation, nothing read back.
 * HKL_E_INVALID: K outside [1, 4096], n_rows < 0, obs_ld < 18, out_col < 0, out_ld < out_col + 4, a null params /
 * packs / obs / out, or null scratch with policy given. */
#define HKL_ACT_WIDE_MAX_POLICIES 4096
typedef struct {
  int32_t n_policies, n_rows;
  const float *params, *packs;
  const float *obs;
  int64_t obs_ld;
  const int32_t *policy;
  float *out;
  int64_t out_ld;
  int32_t out_col;
  int32_t *order, *counts, *offsets, *tiles;
} hkl_act_wide_io;
int hkl_act_wide_io_size(void);
int hkl_act_wide(const hkl_act_wide_io *io, void *stream);

/* ---- twin-critic inference (hockey_amd/value.py) ----
 * The clipped double-Q value of a TD3 agent outside the learner, one launch for n_rows rows:
 *   Q mode (act given):   q_k[i] = Q_k(obs[i * obs_ld .. + 18), unscale(act[i * act_ld .. + 4)))
 *   V mode (act == NULL): a = tanh(actor(obs[i])) as hkl_act computes it, q_k[i] = Q_k(obs[i], unscale(a)) -- the
 *                         critic step's target path with zero noise; the action stays in registers.  act_out
 *                         (optional) receives a in act_out[i * act_out_ld .. + 4).
 * qmin[i] = fminf(q1[i], q2[i]).  unscale is TwinQNetwork._unscale_action with act_low / act_range, as in
 * hkl_critic_io.  The three networks' packs are written by hkl_pack (actor n_in 18 / n_out 4, critics 22 / 1); the
 * actor is read in V mode only.  Any of q1 / q2 / qmin / act_out may be NULL, but not all of them.
 *
 * No float of an output outside its n_rows entries (act_out: the rows' four columns) is written.  A row's results do
 * not depend on the other rows or on its position (bit for bit).  Asynchronous on stream, graph-capturable, no host
 * synchronisation; n_rows == 0 launches nothing.  HKL_E_INVALID (hkl_last_error says which): n_rows < 0, obs_ld < 18,
 * act given with act_ld < 4, act_out given together with act or with act_out_ld < 4, a null obs, a null pack or
 * weight pointer of a network the mode reads, all four outputs null. */
typedef struct {
  int32_t n_rows;
  hkl_net actor;
  hkl_net q[2];
  const float *obs;
  int64_t obs_ld;
  const float *act;
  int64_t act_ld;
  float act_low[4], act_range[4];
  float *q1, *q2, *qmin;
  float *act_out;
  int64_t act_out_ld;
} hkl_value_io;
int hkl_value_io_size(void);
int hkl_value(const hkl_value_io *io, void *stream);

#ifdef __cplusplus
}
#endif
#endif

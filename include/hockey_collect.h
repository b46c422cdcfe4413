/* hockey_collect.h -- collection on the device, of the learner library (libhockey_learner.so): included by
 * hockey_learner.h, which defines HKL_GROUP_MAX and the error codes this header uses; include that one. */
#ifndef HOCKEY_COLLECT_H
#define HOCKEY_COLLECT_H
#ifndef HOCKEY_LEARNER_H
#error "include hockey_learner.h"
#endif

/* ---- collection (hockey_amd/collect.py; csrc/hkl_collect.h) ----
 * What a training step does around the step kernel besides acting: player 2's opponent draw before it (hkl_opp_draw)
 * and the replay store with its bookkeeping after it (hkl_collect), for S = n_rows / rows_per_member members side by
 * side, 1 <= S <= HKL_GROUP_MAX: member m owns rows [m n, (m + 1) n), n = rows_per_member, local(i) = i - m n.  Both
 * calls are asynchronous on stream, graph-capturable, read nothing back and consist of kernel launches only (no memset
 * node), so a capture is a line of kernel nodes.  Nothing read from device memory is used as an address before it is
 * range-checked.
 *
 * hkl_opp_draw -- opponent_manager.py's per-step choice, per row.  Two Philox4x32-10 blocks per row, key = seeds[m] ^
 * purpose, counter = (local lo, local hi, calls[m] lo, calls[m] hi): a function of the member's seed, the row's index
 * inside the member and the member's call counter, never of the row's position in the batch.  With (x, y, z, w) the
 * HKL_COLLECT_KEY_OPP block, u24(v) = (v >> 8) 2^-24 (float) and u53(a, b) = (((a << 32) | b) >> 11) 2^-53 (double):
 *
 *   u_sp = u24(x), u_bot = u24(y), u_snap = u53(z, w);   p_self = probs[m][0], p_strong = probs[m][1]
 *   L = min(max(len[m], 0), pmax);  total = the float64 sum of scores[m][0 .. L) in index order
 *   can_sp = L > 0 && total is finite && total > 0
 *   sp     = can_sp && u_sp < p_self;   strong = !sp && u_bot < p_strong;   weak = !sp && !strong
 *   k      = the first k < L with (float64 sum of scores[m][0 .. k]) > u_snap * total (one rounded product), else L - 1
 *   policy2[i] = sp ? HKL_P2_EXTERNAL : strong ? HKL_P2_STRONG : HKL_P2_WEAK   (the step kernel's HK_POLICY_* ids)
 *   policy[i]  = sp ? slots[m][k] : -1      (stored as read, never used as an address; hkl_act_wide skips a bad slot)
 *   snap[i]    = sp ? m pmax + k : -1
 *   opp_inc[i][c] = 0.2 * u53 of word pair c of the HKL_COLLECT_KEY_PHASE block   (optional: BasicOpponent's phase
 *                   increments, hk_step_io.opp_inc)
 *   counts[m][0 .. 3] += (strong, weak, sp) and snap_counts[snap[i]] += 1 over the rows with alive[i] != 0
 *                   (alive == NULL: every row): integer atomics, so the sums do not depend on the order
 * Every row is drawn and written, alive or not.  After the draw a one-workgroup kernel stores calls[m] += 1; the draw
 * workgroups only read it.  HKL_E_INVALID: null io, n_rows <= 0, rows_per_member <= 0, n_rows no multiple of
 * rows_per_member, S outside [1, HKL_GROUP_MAX], pmax < 1, a null seeds / calls / probs / len / scores / slots /
 * policy2 / policy / snap / counts / snap_counts. */
#define HKL_COLLECT_KEY_OPP 0x6F70706F6E656E74ull /* "opponent" */
#define HKL_COLLECT_KEY_PHASE 0x7068617365ull     /* "phase" */
enum { HKL_P2_EXTERNAL = 0, HKL_P2_WEAK = 2, HKL_P2_STRONG = 3 };
typedef struct {
  int32_t n_rows, rows_per_member, pmax, reserved;
  const uint64_t *seeds; /* device [S] */
  int64_t *calls;        /* device [S] */
  const float *probs;    /* device [S][2]: p_self, p_strong */
  const int32_t *len;    /* device [S]: the member's snapshots, 0 without self-play */
  const float *scores;   /* device [S][pmax] */
  const int32_t *slots;  /* device [S][pmax]: bank slots */
  const uint8_t *alive;  /* device [n_rows], or NULL */
  uint8_t *policy2;      /* device [n_rows] */
  int32_t *policy, *snap; /* device [n_rows] */
  double *opp_inc;       /* device [n_rows][2], or NULL */
  int64_t *counts;       /* device [S][3] */
  int64_t *snap_counts;  /* device [S pmax] */
} hkl_opp_draw_io;
int hkl_opp_draw_io_size(void);
int hkl_opp_draw(const hkl_opp_draw_io *io, void *stream);

/* hkl_collect -- everything after the step: store_step + PopulationRing.push + the mix's outcome tally + the
 * episode-reward and step accumulators + the survivors' count, and the copies that keep the step's outputs.  Member
 * m's ring is rows [m cap, (m + 1) cap) of the columns s [.][18], a [.][4], r, s2 [.][18], d.  "alive" below is the
 * value before the call (alive == NULL: every row is alive and nothing of alive / count is written):
 *
 *   rank(i) = alive rows j < i of the same member;  cnt[m] = the member's alive rows
 *   ok(m)   = 0 <= pos[m] < cap                              (a member that fails it stores nothing and keeps pos / size)
 *   alive row i of an ok member: dst = m cap + (pos[m] + rank(i)) % cap;
 *       s[dst] = obs[i], a[dst] = act[i act_ld + 0 .. 4), r[dst] = reward[i], s2[dst] = obs_next[i], d[dst] = (float)done[i]
 *   push_pos[m] = ok ? pos[m] : 0;  push_n[m] = ok ? cnt[m] : 0;  then, for an ok member,
 *       pos[m] = (pos[m] + cnt[m]) % cap,  size[m] = min(max(size[m], 0) + cnt[m], cap)
 *   ep_reward[i] = ep_reward[i] + (alive ? reward[i] : 0)   (one rounded float sum)
 *   tally[snap[i]][reward[i] > 0 ? 0 : 1] += 1 for an alive row with done[i] != 0 and 0 <= snap[i] < S pmax
 *   steps[m] += cnt[m];   live[m] += cnt[m] > 0 (optional);   alive[i] &= !done[i];   count[m] = the member's alive
 *       rows after that
 *   keep_obs[i] = obs_next[i], keep_obs2[i] = obs2_next[i]  (each optional; keep_obs2 needs obs2_next)
 *
 * The contents and the wrap-around are PopulationRing.push's on store_step's rows (a member's rows stay in arena
 * order); push_pos, push_n and size are the device arrays hkl_per_push_group takes, which a prioritized population calls
 * next.  keep_obs may be obs itself (and keep_obs2 any buffer but obs2_next): every float of a row is read and only then
 * overwritten, by the one thread that owns that float.  No other argument may overlap another.
 *
 * Launches: alive == NULL: one (rank is local; the member's last workgroup to finish, found by a ticket in
 * scratch, commits pos / size / steps).  alive given: three (count per workgroup, scan per member, store).  The
 * number does not depend on S, n_rows or anything on the device.  scratch: device int32 [hkl_collect_scratch_ints(n_rows,
 * rows_per_member)], zero before the first call; a call leaves the ticket words zero.
 * HKL_E_INVALID: null io, n_rows <= 0, rows_per_member <= 0, n_rows no multiple of rows_per_member, S outside
 * [1, HKL_GROUP_MAX], pmax < 1, cap < 1, rows_per_member > cap, act_ld < 4, a null obs / act / obs_next / reward / done
 * / ring column / pos / size / ep_reward / push_pos / push_n / steps / scratch, snap without tally, alive without
 * count, keep_obs2 without obs2_next. */
typedef struct {
  int32_t n_rows, rows_per_member, pmax, reserved;
  const float *obs;       /* device [n_rows][18]: the observation before the step */
  const float *act;       /* device rows of act_ld floats: columns 0 .. 3 are stored */
  int64_t act_ld;
  const float *obs_next;  /* device [n_rows][18] */
  const float *obs2_next; /* device [n_rows][18], or NULL */
  const float *reward;    /* device [n_rows] */
  const uint8_t *done;    /* device [n_rows] */
  const int32_t *snap;    /* device [n_rows], or NULL: no tally */
  uint8_t *alive;         /* device [n_rows], or NULL */
  float *s, *a, *r, *s2, *d; /* the ring columns, S cap rows */
  int64_t cap;
  int64_t *pos, *size;    /* device [S] */
  float *ep_reward;       /* device [n_rows] */
  int64_t *tally;         /* device [S pmax][2] */
  int64_t *push_pos, *push_n; /* device [S] */
  int32_t *count;         /* device [S] */
  int64_t *steps;         /* device [S] */
  int64_t *live;          /* device [S], or NULL: the calls in which the member had an alive row */
  float *keep_obs, *keep_obs2; /* device [n_rows][18], or NULL */
  int32_t *scratch;
} hkl_collect_io;
int hkl_collect_io_size(void);
int64_t hkl_collect_scratch_ints(int32_t n_rows, int32_t rows_per_member);
int hkl_collect(const hkl_collect_io *io, void *stream);

#endif

/* hockey_eval.h -- evaluation on the device, of the learner library (libhockey_learner.so): included by
 * hockey_learner.h, which defines the error codes this header uses; include that one. */
#ifndef HOCKEY_EVAL_H
#define HOCKEY_EVAL_H
#ifndef HOCKEY_LEARNER_H
#error "include hockey_learner.h"
#endif

/* ---- evaluation (hockey_amd/evaluator.py; csrc/hkl_eval.h) ----
 * The accounting of hockey_amd.evaluate.evaluate()'s loop for C = n_rows / rows_per_cell cells side by side, 1 <= C <=
 * HKL_EVAL_CELLS_MAX (the cell is blockIdx.y; HKL_GROUP_MAX does not apply).  A cell is one (player 1 policy, player 2
 * opponent, seed) combination playing n = rows_per_cell games: cell c owns rows [c n, (c + 1) n), local(i) = i - c n.
 * The three calls are asynchronous on stream, graph-capturable, read nothing back and consist of kernel launches only
 * (no memset node).  Nothing read from device memory is used as an address.
 *
 *   inc(c, local, t)[k] = 0.2 * u53 of word pair k of the Philox4x32-10 block with key seeds[c] ^ HKL_EVAL_KEY_PHASE and
 *   counter (local lo, local hi, t lo, t hi), u53(a, b) = (((a << 32) | b) >> 11) 2^-53 (double): hkl_opp_draw's phase
 *   draw under a key of its own; a function of the cell's seed, the row's index inside the cell and the step, never of
 *   the row's position in the batch.
 *
 * hkl_eval_begin -- live = 1, ret = +0.0, length = 0, winner = 0, count[c] = n, step[0] = 0, opp_inc[i] = inc(c, local,
 *   0) (opp_inc optional here and in hkl_eval_step).
 *
 * hkl_eval_step -- after a step of the env, with t = step[0] before the call.  A row with live[i] != 0:
 *     ret[i] += (double)reward[i]   (one rounded sum);   length[i] += 1;
 *     if done[i] != 0: winner[i] = f > 0 ? 1 : f < 0 ? -1 : 0 with f = info[i info_ld] (a NaN gives 0), live[i] = 0
 *   A row with live[i] == 0 keeps every word.  count[c] -= the cell's rows that finished in this call (integer atomics,
 *   at most one per wave, so the value does not depend on the order): after hkl_eval_begin and any number of steps,
 *   count[c] is the cell's live rows.  Every row, live or not, gets opp_inc[i] = inc(c, local, t + 1).  A trailing
 *   one-workgroup kernel stores step[0] = t + 1; the row workgroups only read it.
 *
 * hkl_eval_fold -- one workgroup of 256 per cell; a row is finished when live[i] == 0.
 *     outcomes[c][0 .. 4) = the finished rows with winner +1, 0, -1, then the live rows
 *     length_sum[c]       = the integer sum of length over the finished rows
 *     return_sum[c]       = float64, in a fixed order: lane l sums ret of the cell's finished rows j = l, l + 256, ... in
 *                           increasing j from +0.0 into p[l]; then for s = 128, 64, ..., 1: p[l] += p[l + s] for l < s;
 *                           the result is p[0]
 *
 * Containment: a non-finite reward or info value reaches only that row's ret / winner and its cell's return_sum; no
 * count and no other cell.
 * HKL_E_INVALID: null io, n_rows <= 0, rows_per_cell <= 0, n_rows no multiple of rows_per_cell, C outside [1,
 * HKL_EVAL_CELLS_MAX], info_ld < 1, a null array that the call reads or writes (opp_inc excepted) -- begin: seeds, step,
 * live, ret, length, winner, count; step: those and reward, done, info; fold: live, ret, length, winner, outcomes,
 * length_sum, return_sum. */
#define HKL_EVAL_KEY_PHASE 0x6576616C70686173ull /* "evalphas" */
#define HKL_EVAL_CELLS_MAX 65535
typedef struct {
  int32_t n_rows, rows_per_cell;
  int64_t info_ld;
  const uint64_t *seeds; /* device [C] */
  int64_t *step;         /* device [1] */
  const float *reward;   /* device [n_rows] */
  const uint8_t *done;   /* device [n_rows] */
  const float *info;     /* device rows of info_ld floats: column 0 is the winner */
  uint8_t *live;         /* device [n_rows] */
  double *ret;           /* device [n_rows] */
  int32_t *length;       /* device [n_rows] */
  int8_t *winner;        /* device [n_rows] */
  int32_t *count;        /* device [C] */
  double *opp_inc;       /* device [n_rows][2], or NULL */
  int64_t *outcomes;     /* device [C][4]: fold output */
  int64_t *length_sum;   /* device [C]: fold output */
  double *return_sum;    /* device [C]: fold output */
} hkl_eval_io;
int hkl_eval_io_size(void);
int hkl_eval_begin(const hkl_eval_io *io, void *stream);
int hkl_eval_step(const hkl_eval_io *io, void *stream);
int hkl_eval_fold(const hkl_eval_io *io, void *stream);

#endif

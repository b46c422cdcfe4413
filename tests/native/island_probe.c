/* Island probe: the CPU oracle with a recorder on every island / TOI velocity solve (test infrastructure only;
 * built by tests/wave_zoo.py next to the oracle library, with the oracle's flags).
 *
 * For each arena of a batched step (hkov_step) it records up to HKP_MAXSOLVE island solves with at least one
 * contact, in solve order -- the order in which the kernel lays a lane's contacts into its slots:
 *   contact count; the period-4 exit iteration `cur` of the kernel's velocity loops (hk_velocity.h): the first
 *   k = 3 (mod 4), k >= 7, whose state (island body velocities, contact impulses) equals the state at k - 4, plus
 *   1, else 180; per contact (the first 4): island-local body indices iA / iB, whether body A is dynamic, points.
 * and of the step's TOI mini-island solves: how many, the largest, how many of exactly 2 and of more than 2
 * contacts.  Record layout (int32, HKP_REC words per arena): see the HKP_* offsets below and tests/wave_zoo.py.
 *
 * Exports hkp_arm / hkp_disarm; every other symbol is the oracle's own. */
#define HKO_VEL_HOOK(S, Vl, nb, it, toi) hkp_hook((const void *)(S), (const void *)(Vl), (nb), (it), (toi))
static void hkp_hook(const void *S, const void *Vl, int nb, int it, int toi);
#define HKO_ARENA_HOOK(i) hkp_arena(i)
#include <stdint.h>
static void hkp_arena(int64_t i);
#include "../../oracle/hk_oracle.c"

#define HKP_MAXW 96
#define HKP_MAXSOLVE 4
#define HKP_NS 0       /* island solves with >= 1 contact (all of them, also beyond HKP_MAXSOLVE) */
#define HKP_NCONT 1    /* their contacts in total */
#define HKP_TOI 2      /* TOI mini-island solves */
#define HKP_TOI_MAX 3  /* contacts of the largest */
#define HKP_TOI_N2 4   /* mini-islands of exactly 2 contacts */
#define HKP_TOI_BIG 5  /* mini-islands of more than 2 contacts */
#define HKP_HEAD 6
#define HKP_SOLVE 18   /* n, cur, 4 x (iA, iB, dynA, points) */
#define HKP_REC (HKP_HEAD + HKP_MAXSOLVE * HKP_SOLVE)

static __thread uint32_t hkp_x[VEL_ITERS][HKP_MAXW];
static __thread int64_t hkp_cur_arena = -1;
static int32_t *hkp_buf;
static int64_t hkp_n;

int hkp_rec_words(void) { return HKP_REC; }
void hkp_arm(int32_t *buf, int64_t n) {
  hkp_n = n;
  hkp_buf = buf;
}
void hkp_disarm(void) { hkp_buf = NULL; }

static void hkp_arena(int64_t i) { hkp_cur_arena = i; }

static void hkp_hook(const void *Sv, const void *Vlv, int nb, int it, int toi) {
  const csolver *S = (const csolver *)Sv;
  const velv *Vl = (const velv *)Vlv;
  if (!hkp_buf || S->n == 0) return;
  int n = 0;
  uint32_t *x = hkp_x[it];
  for (int i = 0; i < nb && n + 3 <= HKP_MAXW; ++i) {
    memcpy(&x[n++], &Vl[i].v.x, 4);
    memcpy(&x[n++], &Vl[i].v.y, 4);
    memcpy(&x[n++], &Vl[i].w, 4);
  }
  for (int i = 0; i < S->n; ++i)
    for (int j = 0; j < S->vc[i].count && n + 2 <= HKP_MAXW; ++j) {
      memcpy(&x[n++], &S->vc[i].p[j].ni, 4);
      memcpy(&x[n++], &S->vc[i].p[j].ti, 4);
    }
  if (it != VEL_ITERS - 1 || hkp_cur_arena < 0 || hkp_cur_arena >= hkp_n) return;
  int32_t *r = hkp_buf + hkp_cur_arena * HKP_REC;
  if (toi) {
    r[HKP_TOI] += 1;
    if (S->n > r[HKP_TOI_MAX]) r[HKP_TOI_MAX] = S->n;
    if (S->n == 2) r[HKP_TOI_N2] += 1;
    if (S->n > 2) r[HKP_TOI_BIG] += 1;
    return;
  }
  int cur = VEL_ITERS;
  for (int k = 7; k < VEL_ITERS; k += 4)
    if (!memcmp(hkp_x[k], hkp_x[k - 4], 4 * (size_t)n)) { cur = k + 1; break; }
  const int k = r[HKP_NS]++;
  r[HKP_NCONT] += S->n;
  if (k >= HKP_MAXSOLVE) return;
  int32_t *s = r + HKP_HEAD + k * HKP_SOLVE;
  s[0] = S->n;
  s[1] = cur;
  for (int i = 0; i < 4 && i < S->n; ++i) {
    s[2 + 4 * i] = S->vc[i].iA;
    s[3 + 4 * i] = S->vc[i].iB;
    s[4 + 4 * i] = S->vc[i].mA != 0.0f;
    s[5 + 4 * i] = S->vc[i].count;
  }
}

// hk_learner.hip -- the batched TD3 learner (BASELINE C5) as fused fp32 MFMA kernels for gfx950.
//
// One learner update of rl/td3/learner.py:55-218 at a large batch B (C5 draws 16 384 samples per update):
//   critic_step   target policy smoothing + clipped double-Q target (compute_target, :75-112), both critics'
//                 forward, the weighted smooth-L1 loss (rl/utils/torch_utils.py:12-24) and its backward through
//                 both critics down to the first layer -- one launch, B / 64 workgroups of 4 waves, 16 samples
//                 per wave;
//   actor_step    actor forward, Q1 of the updated critic on (s, actor(s)), -mean Q1 backward through Q1 to the
//                 action and through the actor (update_actor, :138-175) -- one launch;
//   wgrad         the weight gradients dW = dZ^T X (the reduction over the batch) as split-K MFMA tiles;
//   adam          per-parameter reduction of the gradient slabs in a fixed order + torch.optim.Adam's update
//                 (lr, betas (0.9, 0.999), eps, L2 weight decay; rl/td3/agent.py:174-182), on actor updates with
//                 soft_update (:196-218) folded in;
//   pack          re-lays the changed weights out for the MFMA operands (polyak: soft_update as its own launch).
//   per_*         prioritized replay on per-block float64 sums: slots, importance weights, the priority write-back and
//                 the push rule without a pass over the ring; their *_group forms run up to 64 rings per launch, the
//                 push with its sizes read on the device.
//   act           acting: the actor forward of actor_step over a bank of policies, a different one per row, the rows
//                 grouped by policy on the device.
//   explore       act with TD3.act's exploration (annealed noise, random phase) as the acting tile's epilogue.
//   collect       what a training step does around the step kernel: the opponent draw and the replay store.
//   eval          the evaluation loop's accounting for many (policy, opponent, seed) cells side by side, and its fold.
//   value         twin-critic inference: Q_k(s, a), or V(s) = min Q_k(s, actor(s)) with the action kept in registers.
//
// The library's only translation unit: the kernels live in the headers below, included in the order of their
// definition (the code object keeps it); the C ABI of include/hockey_learner.h follows, one section per header.
#include "hkl_mlp.h"    // Tile, Net, gemm_in / gemm256 / gemm_out, head1, back_out, the reductions
#include "hkl_td3.h"    // Philox sampler, critic step, actor step, wgrad, adam, polyak, pack
#include "hkl_per.h"    // prioritized replay
#include "hkl_act.h"    // hkl_act / hkl_act_wide
#include "hkl_explore.h"  // hkl_explore: hkl_act with the exploration epilogue
#include "hkl_collect.h"  // hkl_opp_draw, hkl_collect
#include "hkl_eval.h"   // hkl_eval_begin / hkl_eval_step / hkl_eval_fold
#include "hkl_value.h"  // hkl_value

using namespace hkl;

// ------------------------------------------------------------------------------------------------ host helpers
// One error path: every refused call goes through invalid() (or bad_group / bad_member, which name the member), every
// launch site ends in launched(), so hkl_last_error() always describes the call that just failed.
static thread_local char g_err[256];
static int fail(hipError_t e, const char *who) {
  snprintf(g_err, sizeof g_err, "%s: %s", who, hipGetErrorString(e));
  return HKL_E_DEVICE;
}
static int invalid(const char *who, const char *what) {
  snprintf(g_err, sizeof g_err, "%s: %s", who, what);
  return HKL_E_INVALID;
}
static int launched(const char *who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, who);
}
static unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// One validator per struct: bad_*(x) is what is wrong with x, or nullptr.  The single call checks its struct (bad_io);
// the grouped call the group, every member of the host copy with the same validator and that the members agree on what
// sizes the grid (bad_members, differs_*(member, member 0)).  Where the single form is looser, bad_* takes the Form.
enum Form : bool { kSingle = false, kGrouped = true };

template <class IO, class Bad>
static int bad_io(const char *who, const IO *io, Bad bad) {
  if (!io) return invalid(who, "null io");
  const char *w = bad(*io);
  return w ? invalid(who, w) : 0;
}
static int bad_group(const char *who, const void *host, const void *dev, int n_members) {
  if (n_members < 1 || n_members > HKL_GROUP_MAX)
    snprintf(g_err, sizeof g_err, "%s: n_members %d outside [1, %d]", who, n_members, HKL_GROUP_MAX);
  else if (!host || !dev) snprintf(g_err, sizeof g_err, "%s: null %s array", who, host ? "dev" : "host");
  else return 0;
  return HKL_E_INVALID;
}
static int bad_member(const char *who, int m, const char *what) {
  snprintf(g_err, sizeof g_err, "%s: member %d: %s", who, m, what);
  return HKL_E_INVALID;
}
template <class IO, class Bad, class Differs>
static int bad_members(const char *who, const IO *host, const void *dev, int n_members, Bad bad, Differs differs) {
  if (const int rc = bad_group(who, host, dev, n_members)) return rc;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad(host[m])) return bad_member(who, m, w);
    if (const char *w = differs(host[m], host[0])) return bad_member(who, m, w);
  }
  return 0;
}
template <class IO>
static const char *differs_batch(const IO &a, const IO &b) {
  return a.batch != b.batch ? "batch differs from member 0's" : nullptr;
}

// ------------------------------------------------------------------------------------------------ C ABI: TD3 learner
static const char *bad_net(const hkl_net &n) {
  return (!n.w1 || !n.b1 || !n.w2 || !n.b2 || !n.w3 || !n.b3 || !n.pack) ? "null network pointer" : nullptr;
}
static const char *bad_nets(const hkl_net *nets, int n_nets) {
  if (n_nets < 1 || n_nets > 4) return "n_nets outside [1, 4]";
  for (int k = 0; k < n_nets; ++k)
    if (const char *w = bad_net(nets[k])) return w;
  return nullptr;
}
static const char *bad_batch(int64_t b) { return (b <= 0 || b % CHUNK) ? "batch is not a positive multiple of 256" : nullptr; }
// kSingle: any positive batch (sample_body guards e < batch, and the prioritized replay tests draw odd batches through
// hkl_sample); kGrouped: the grid is batch / 256, as every other grouped learner call's
template <Form F>
static const char *bad_sample(const hkl_sample_io &io) {
  if (const char *w = F == kGrouped ? bad_batch(io.batch) : io.batch <= 0 ? "batch is not positive" : nullptr) return w;
  return (!io.counter || !io.size || !io.idx || !io.noise) ? "null counter / size / idx / noise" : nullptr;
}
static const char *bad_critic(const hkl_critic_io &io) {
  if (const char *w = bad_batch(io.batch)) return w;
  if (!io.idx || !io.ring_s || !io.ring_a || !io.ring_r || !io.ring_s2 || !io.ring_d || !io.noise)
    return "null idx / ring column / noise";
  for (const hkl_net *n : {&io.target_actor, &io.target_q[0], &io.target_q[1], &io.q[0], &io.q[1]})
    if (const char *w = bad_net(*n)) return w;
  if (!io.x0 || !io.p_loss) return "null x0 / p_loss";
  for (int k = 0; k < 2; ++k)
    if (!io.h1[k] || !io.dz1[k] || !io.dz2[k] || !io.p_dw3[k] || !io.p_db3[k]) return "null h1 / dz1 / dz2 / p_dw3 / p_db3";
  return nullptr;
}
static const char *bad_actor(const hkl_actor_io &io) {
  if (const char *w = bad_batch(io.batch)) return w;
  if (!io.idx || !io.ring_s) return "null idx / ring_s";
  if (bad_net(io.actor) || bad_net(io.q1)) return "null network pointer";
  if (!io.x0 || !io.h1 || !io.h2 || !io.dz1 || !io.dz2 || !io.p_dw3 || !io.p_db3 || !io.p_loss)
    return "null x0 / h1 / h2 / dz1 / dz2 / p_dw3 / p_db3 / p_loss";
  return nullptr;
}
static const char *bad_adam(const hkl_adam_io &io) {
  if (io.n_seg < 1 || io.n_seg > HKL_MAX_SEG) return "n_seg outside [1, HKL_MAX_SEG]";
  if (io.loss_src && (!io.loss_sum || !io.loss_count)) return "loss partials without loss_sum / loss_count";
  if (!io.step) return "null step";
  for (int s = 0; s < io.n_seg; ++s)
    if (!io.seg[s].param || !io.seg[s].m || !io.seg[s].v || !io.seg[s].src || (io.polyak && !io.seg[s].target))
      return "null segment pointer";
  return nullptr;
}
static const char *differs_adam(const hkl_adam_io &a, const hkl_adam_io &b) {
  if (a.n_seg != b.n_seg) return "n_seg differs from member 0's";
  for (int s = 0; s < a.n_seg; ++s)
    if (a.seg[s].rows != b.seg[s].rows || a.seg[s].cols != b.seg[s].cols)
      return "a segment's rows x cols differ from member 0's";
  return nullptr;
}
static int64_t adam_params(const hkl_adam_io &io) {
  int64_t n = 0;
  for (int s = 0; s < io.n_seg; ++s) n += (int64_t)io.seg[s].rows * io.seg[s].cols;
  return n;
}
static const char *bad_wgrad(int n_jobs, int64_t batch) {
  return (n_jobs < 1 || n_jobs > 4) ? "job count outside [1, 4]" : bad_batch(batch);
}
static const char *bad_wgrad_jobs(const hkl_wgrad_job *jobs, int n_jobs) {
  for (int k = 0; k < n_jobs; ++k)
    if (!jobs[k].dz || !jobs[k].x || !jobs[k].slab) return "null dz / x / slab of a job";
  return nullptr;
}
// samples per split-K chunk (include/hockey_learner.h hkl_wgrad).  dW2 (k width 256): 512-sample chunks when the batch
// allows and two or more networks fill the chip (fewer partial slabs for adam to add); one network (the actor: 4 x
// B / 512 tiles at 512 are half the workgroups the chip holds at C5's batch) or dW1 (k width 32, a small tile per
// block): 256, for more blocks
static int wg_chunk_size(int n_jobs, int k_width, int64_t batch) {
  return (k_width == 256 && n_jobs >= 2 && batch % 512 == 0) ? 512 : 256;
}
static WgJobs wg_jobs(const hkl_wgrad_job *jobs, int n_jobs, int k_width, int64_t batch) {
  WgJobs J{};
  for (int k = 0; k < n_jobs; ++k) J.job[k] = WgJob{jobs[k].dz, jobs[k].x, jobs[k].slab, jobs[k].bias_slab, k_width};
  J.chunk_size = wg_chunk_size(n_jobs, k_width, batch);
  J.chunks = (int)(batch / J.chunk_size);
  return J;
}

extern "C" {

const char *hkl_last_error(void) { return g_err; }
int hkl_pack_floats(void) { return kPackFloats; }

int hkl_pack(const hkl_net *nets, int n_nets, int64_t *step, void *stream) {
  const char *who = "hkl_pack";
  if (!nets) return invalid(who, "null nets");
  if (const char *w = bad_nets(nets, n_nets)) return invalid(who, w);
  hkl_pack_io io{};
  for (int k = 0; k < n_nets; ++k) io.net[k] = nets[k];
  io.step = step;
  hipLaunchKernelGGL(pack_kernel, dim3(blocks(kPackFloats, 256), n_nets), dim3(256), 0, (hipStream_t)stream, io);
  return launched(who);
}

int hkl_critic_step(const hkl_critic_io *io, void *stream) {
  const char *who = "hkl_critic_step";
  if (const int rc = bad_io(who, io, bad_critic)) return rc;
  hipLaunchKernelGGL(critic_step_kernel, dim3(io->batch / 64), dim3(WG), 0, (hipStream_t)stream, *io);
  return launched(who);
}

int hkl_actor_step(const hkl_actor_io *io, void *stream) {
  const char *who = "hkl_actor_step";
  if (const int rc = bad_io(who, io, bad_actor)) return rc;
  hipLaunchKernelGGL(actor_step_kernel, dim3(io->batch / 64), dim3(WG), 0, (hipStream_t)stream, *io);
  return launched(who);
}

int hkl_wgrad(const hkl_wgrad_job *jobs, int n_jobs, int k_width, int64_t batch, void *stream) {
  const char *who = "hkl_wgrad";
  if (!jobs) return invalid(who, "null jobs");
  if (const char *w = bad_wgrad(n_jobs, batch)) return invalid(who, w);
  if (k_width != 256 && k_width != XP) return invalid(who, "k_width is neither 256 nor 32");
  if (const char *w = bad_wgrad_jobs(jobs, n_jobs)) return invalid(who, w);
  const WgJobs J = wg_jobs(jobs, n_jobs, k_width, batch);
  const unsigned z = (unsigned)(J.chunks * n_jobs);
  if (k_width == 256) hipLaunchKernelGGL(wgrad_kernel<128>, dim3(2, 2, z), dim3(WG), 0, (hipStream_t)stream, J);
  else hipLaunchKernelGGL(wgrad_kernel<32>, dim3(2, 1, z), dim3(WG), 0, (hipStream_t)stream, J);
  return launched(who);
}

int hkl_wgrad_pair(const hkl_wgrad_job *wide, int n_wide, const hkl_wgrad_job *narrow, int n_narrow, int64_t batch,
                   void *stream) {
  const char *who = "hkl_wgrad_pair";
  if (!wide || !narrow) return invalid(who, "null wide / narrow jobs");
  if (const char *w = bad_wgrad(n_wide, batch)) return invalid(who, w);
  if (const char *w = bad_wgrad(n_narrow, batch)) return invalid(who, w);
  if (const char *w = bad_wgrad_jobs(wide, n_wide)) return invalid(who, w);
  if (const char *w = bad_wgrad_jobs(narrow, n_narrow)) return invalid(who, w);
  const WgJobs W = wg_jobs(wide, n_wide, 256, batch), N = wg_jobs(narrow, n_narrow, XP, batch);
  const int nw = 4 * W.chunks * n_wide, nn = 2 * N.chunks * n_narrow;
  hipLaunchKernelGGL(wgrad_pair_kernel, dim3((unsigned)(nw + nn)), dim3(WG), 0, (hipStream_t)stream, W, N, nw);
  return launched(who);
}

int hkl_adam(const hkl_adam_io *io, void *stream) {
  const char *who = "hkl_adam";
  if (const int rc = bad_io(who, io, bad_adam)) return rc;
  hipLaunchKernelGGL(adam_kernel, dim3(blocks(adam_params(*io), 256)), dim3(256), 0, (hipStream_t)stream, *io);
  return launched(who);
}

int hkl_polyak(float *target, const float *param, int64_t n, float rho, float tau, void *stream) {
  const char *who = "hkl_polyak";
  if (n <= 0) return invalid(who, "n is not positive");
  hipLaunchKernelGGL(polyak_kernel, dim3(blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, target, param, n, rho, tau);
  return launched(who);
}

int hkl_tanh_probe(const float *x, float *y, int64_t n, void *stream) {
  const char *who = "hkl_tanh_probe";
  if (n <= 0) return invalid(who, "n is not positive");
  hipLaunchKernelGGL(tanh_probe_kernel, dim3(blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return launched(who);
}

int hkl_sample(const hkl_sample_io *io, void *stream) {
  const char *who = "hkl_sample";
  if (const int rc = bad_io(who, io, bad_sample<kSingle>)) return rc;
  hipLaunchKernelGGL(sample_kernel, dim3(blocks(io->batch, 256)), dim3(256), 0, (hipStream_t)stream, *io);
  return launched(who);
}

// ---- grouped forms (include/hockey_learner.h): the host copy is checked, then one launch reads the device copy
int hkl_sample_group(const hkl_sample_io *host, const hkl_sample_io *dev, int n_members, void *stream) {
  const char *who = "hkl_sample_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_sample<kGrouped>, differs_batch<hkl_sample_io>)) return rc;
  hipLaunchKernelGGL(sample_group_kernel, dim3((unsigned)(host[0].batch / 256), n_members), dim3(256), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_critic_step_group(const hkl_critic_io *host, const hkl_critic_io *dev, int n_members, void *stream) {
  const char *who = "hkl_critic_step_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_critic, differs_batch<hkl_critic_io>)) return rc;
  hipLaunchKernelGGL(critic_step_group_kernel, dim3((unsigned)(host[0].batch / 64), n_members), dim3(WG), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_actor_step_group(const hkl_actor_io *host, const hkl_actor_io *dev, int n_members, void *stream) {
  const char *who = "hkl_actor_step_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_actor, differs_batch<hkl_actor_io>)) return rc;
  hipLaunchKernelGGL(actor_step_group_kernel, dim3((unsigned)(host[0].batch / 64), n_members), dim3(WG), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_wgrad_pair_group(const hkl_wgrad_job *wide_host, const hkl_wgrad_job *wide_dev, int n_wide,
                         const hkl_wgrad_job *narrow_host, const hkl_wgrad_job *narrow_dev, int n_narrow, int64_t batch,
                         int n_members, void *stream) {
  const char *who = "hkl_wgrad_pair_group";
  if (const int rc = bad_group(who, wide_host, wide_dev, n_members)) return rc;
  if (const int rc = bad_group(who, narrow_host, narrow_dev, n_members)) return rc;
  if (const char *w = bad_wgrad(n_wide, batch)) return invalid(who, w);
  if (const char *w = bad_wgrad(n_narrow, batch)) return invalid(who, w);
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_wgrad_jobs(wide_host + m * n_wide, n_wide)) return bad_member(who, m, w);
    if (const char *w = bad_wgrad_jobs(narrow_host + m * n_narrow, n_narrow)) return bad_member(who, m, w);
  }
  const int cw = wg_chunk_size(n_wide, 256, batch), cn = wg_chunk_size(n_narrow, XP, batch);  // as hkl_wgrad_pair's
  const int chunks_w = (int)(batch / cw), chunks_n = (int)(batch / cn);
  const WgGroup g{wide_dev, narrow_dev, n_wide, n_narrow, chunks_w, cw, chunks_n, cn, 4 * chunks_w * n_wide};
  const int nn = 2 * chunks_n * n_narrow;
  hipLaunchKernelGGL(wgrad_pair_group_kernel, dim3((unsigned)(g.n_wide + nn), n_members), dim3(WG), 0,
                     (hipStream_t)stream, g);
  return launched(who);
}

int hkl_adam_group(const hkl_adam_io *host, const hkl_adam_io *dev, int n_members, void *stream) {
  const char *who = "hkl_adam_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_adam, differs_adam)) return rc;
  hipLaunchKernelGGL(adam_group_kernel, dim3(blocks(adam_params(host[0]), 256), n_members), dim3(256), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_pack_group(const hkl_pack_io *host, const hkl_pack_io *dev, int n_nets, int n_members, void *stream) {
  const char *who = "hkl_pack_group";
  if (const int rc = bad_group(who, host, dev, n_members)) return rc;
  for (int m = 0; m < n_members; ++m)
    if (const char *w = bad_nets(host[m].net, n_nets)) return bad_member(who, m, w);
  hipLaunchKernelGGL(pack_group_kernel, dim3(blocks(kPackFloats, 256), n_nets, n_members), dim3(256), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ C ABI: prioritized replay
// kGrouped: a member's w is a slice of a shared storage and has to be placed on 16 bytes, since per_load reads a lane's
// sub-chunk as four float4; kSingle: the ring's own allocation is aligned
template <Form F>
static const char *bad_per(const hkl_per &p) {
  if (p.cap <= 0) return "cap is not positive";
  if (!p.w || !p.size || !p.bsum || !p.bmax || !p.bpre || !p.last || !p.bown)
    return "null w / size / bsum / bmax / bpre / last / bown";
  return (F == kGrouped && (uintptr_t)p.w % 16) ? "w is not 16-byte aligned" : nullptr;
}
// Draw: hkl_per_sample, which needs u or counter and takes iw as optional; else hkl_per_weights, which needs iw
template <Form F, bool Draw>
static const char *bad_per_sample(const hkl_per_sample_io &io) {
  if (const char *w = bad_per<F>(io.per)) return w;
  if (io.batch <= 0 || io.batch >= ((int64_t)1 << 31)) return "batch outside [1, 2^31)";
  if (!io.idx) return "null idx";
  if (Draw) return (io.u || io.counter) ? nullptr : "null u and null counter";
  return io.iw ? nullptr : "null iw";
}
template <Form F>
static const char *bad_per_update(const hkl_per_update_io &io) {
  if (const char *w = bad_per<F>(io.per)) return w;
  if (io.batch <= 0 || io.batch >= ((int64_t)1 << 31)) return "batch outside [1, 2^31)";
  return (io.idx && io.td) ? nullptr : "null idx / td";
}
// the members' grids agree: one cap (so one block count) and, where the struct has one, one batch
static const char *differs_cap(const hkl_per &a, const hkl_per &b) {
  return a.cap != b.cap ? "cap differs from member 0's" : nullptr;
}
template <class IO>
static const char *differs_per(const IO &a, const IO &b) {
  const char *w = differs_cap(a.per, b.per);
  return w ? w : differs_batch(a, b);
}
static int64_t per_nblk(const hkl_per &p) { return (p.cap + HKL_PER_BLOCK - 1) / HKL_PER_BLOCK; }
static void per_refresh_launch(const hkl_per &p, int64_t lo, int64_t n, int64_t size_arg, hipStream_t st) {
  const int64_t b0 = lo / HKL_PER_BLOCK, nb = (lo + n - 1) / HKL_PER_BLOCK - b0 + 1;
  hipLaunchKernelGGL(per_refresh_kernel, dim3(blocks(nb, 4)), dim3(256), 0, st, p, b0, nb, size_arg);
}

extern "C" {

int hkl_per_block(void) { return HKL_PER_BLOCK; }

int hkl_per_refresh(const hkl_per *per, int64_t lo, int64_t n, void *stream) {
  const char *who = "hkl_per_refresh";
  if (const int rc = bad_io(who, per, bad_per<kSingle>)) return rc;
  if (lo < 0 || n <= 0 || n > per->cap || lo > per->cap - n) return invalid(who, "[lo, lo + n) is empty or outside the ring");
  per_refresh_launch(*per, lo, n, -1, (hipStream_t)stream);
  return launched(who);
}

int hkl_per_push(const hkl_per *per, int64_t pos, int64_t n, int64_t size_after, void *stream) {
  const char *who = "hkl_per_push";
  if (const int rc = bad_io(who, per, bad_per<kSingle>)) return rc;
  if (pos < 0 || pos >= per->cap || n <= 0 || n > per->cap || size_after < n || size_after > per->cap)
    return invalid(who, "pos outside [0, cap), n outside [1, cap] or size_after outside [n, cap]");
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(per_push_kernel, dim3(1), dim3(1024), 0, st, *per, pos, n, size_after);
  const int64_t head = per->cap - pos < n ? per->cap - pos : n;
  per_refresh_launch(*per, pos, head, size_after, st);
  if (head < n) per_refresh_launch(*per, 0, n - head, size_after, st);
  return launched(who);
}

int hkl_per_weights(const hkl_per_sample_io *io, void *stream) {
  const char *who = "hkl_per_weights";
  if (const int rc = bad_io(who, io, bad_per_sample<kSingle, false>)) return rc;
  hipLaunchKernelGGL(per_iw_kernel, dim3(blocks(io->batch, 1024)), dim3(1024), 0, (hipStream_t)stream, io->per, io->idx,
                     io->iw, io->batch, io->beta);
  return launched(who);
}

int hkl_per_sample(const hkl_per_sample_io *io, void *stream) {
  const char *who = "hkl_per_sample";
  if (const int rc = bad_io(who, io, bad_per_sample<kSingle, true>)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = per_nblk(io->per);
  hipLaunchKernelGGL(per_prefix_kernel, dim3(1), dim3(1024), 0, st, io->per, nblk);
  hipLaunchKernelGGL(per_sample_kernel, dim3(blocks(io->batch, 4)), dim3(256), 0, st, *io, nblk);
  if (io->iw)
    hipLaunchKernelGGL(per_iw_kernel, dim3(blocks(io->batch, 1024)), dim3(1024), 0, st, io->per, io->idx, io->iw,
                       io->batch, io->beta);
  return launched(who);
}

int hkl_per_update(const hkl_per_update_io *io, void *stream) {
  const char *who = "hkl_per_update";
  if (const int rc = bad_io(who, io, bad_per_update<kSingle>)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned g = blocks(io->batch, 256);
  hipLaunchKernelGGL(per_mark_kernel, dim3(g), dim3(256), 0, st, *io);
  hipLaunchKernelGGL(per_write_kernel, dim3(g), dim3(256), 0, st, *io);
  hipLaunchKernelGGL(per_touch_kernel, dim3(blocks(io->batch, 4)), dim3(256), 0, st, *io);
  return launched(who);
}

// ---- grouped forms (include/hockey_learner.h): the single calls' launches with the member in blockIdx.y
int hkl_per_refresh_group(const hkl_per *host, const hkl_per *dev, int n_members, void *stream) {
  const char *who = "hkl_per_refresh_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_per<kGrouped>, differs_cap)) return rc;
  const int64_t nblk = per_nblk(host[0]);
  hipLaunchKernelGGL(per_refresh_group_kernel, dim3(blocks(nblk, 4), n_members), dim3(256), 0, (hipStream_t)stream, dev,
                     nblk);
  return launched(who);
}

int hkl_per_push_group(const hkl_per *host, const hkl_per *dev, const int64_t *pos, const int64_t *n,
                       const int64_t *size_after, int64_t max_n, int n_members, void *stream) {
  const char *who = "hkl_per_push_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_per<kGrouped>, differs_cap)) return rc;
  if (!pos || !n || !size_after) return invalid(who, "null pos / n / size_after array");
  if (max_n < 1 || max_n > host[0].cap) return invalid(who, "max_n outside [1, cap]");
  const hipStream_t st = (hipStream_t)stream;
  // the blocks a push of max_n slots can cover: a head that starts anywhere in a block, a tail that starts at slot 0
  const int64_t nblk = per_nblk(host[0]);
  int64_t n_head = (max_n + HKL_PER_BLOCK - 2) / HKL_PER_BLOCK + 1, n_tail = (max_n - 1 + HKL_PER_BLOCK - 1) / HKL_PER_BLOCK;
  n_head = n_head < nblk ? n_head : nblk;
  n_tail = n_tail < nblk ? n_tail : nblk;
  hipLaunchKernelGGL(per_push_group_kernel, dim3(1, n_members), dim3(1024), 0, st, dev, pos, n, size_after, max_n);
  hipLaunchKernelGGL(per_push_refresh_group_kernel, dim3(blocks(n_head + n_tail, 4), n_members), dim3(256), 0, st, dev,
                     pos, n, size_after, max_n, n_head, n_tail);
  return launched(who);
}

int hkl_per_weights_group(const hkl_per_sample_io *host, const hkl_per_sample_io *dev, int n_members, void *stream) {
  const char *who = "hkl_per_weights_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_per_sample<kGrouped, false>, differs_per<hkl_per_sample_io>))
    return rc;
  hipLaunchKernelGGL(per_iw_group_kernel, dim3(blocks(host[0].batch, 1024), n_members), dim3(1024), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_per_sample_group(const hkl_per_sample_io *host, const hkl_per_sample_io *dev, int n_members, void *stream) {
  const char *who = "hkl_per_sample_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_per_sample<kGrouped, true>, differs_per<hkl_per_sample_io>))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = per_nblk(host[0].per), batch = host[0].batch;
  hipLaunchKernelGGL(per_prefix_group_kernel, dim3(1, n_members), dim3(1024), 0, st, dev, nblk);
  hipLaunchKernelGGL(per_sample_group_kernel, dim3(blocks(batch, 4), n_members), dim3(256), 0, st, dev, nblk);
  // always launched, so that the launch count does not depend on the members: one without iw leaves at once
  hipLaunchKernelGGL(per_iw_group_kernel, dim3(blocks(batch, 1024), n_members), dim3(1024), 0, st, dev);
  return launched(who);
}

int hkl_per_update_group(const hkl_per_update_io *host, const hkl_per_update_io *dev, int n_members, void *stream) {
  const char *who = "hkl_per_update_group";
  if (const int rc = bad_members(who, host, dev, n_members, bad_per_update<kGrouped>, differs_per<hkl_per_update_io>))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t batch = host[0].batch;
  const dim3 g(blocks(batch, 256), n_members);
  hipLaunchKernelGGL(per_mark_group_kernel, g, dim3(256), 0, st, dev);
  hipLaunchKernelGGL(per_write_group_kernel, g, dim3(256), 0, st, dev);
  hipLaunchKernelGGL(per_touch_group_kernel, dim3(blocks(batch, 4), n_members), dim3(256), 0, st, dev);
  return launched(who);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ C ABI: acting
// hkl_act_io and hkl_act_wide_io share every field but the wide form's tile table: max_k is the bank's capacity,
// tiles_ok whether the grouping's tile table is there (hkl_act has none to ask for)
template <class IO>
static const char *bad_act(const IO &io, int max_k, bool tiles_ok) {
  if (io.n_policies < 1 || io.n_policies > max_k) return "n_policies outside the bank's [1, capacity]";
  if (io.n_rows < 0) return "n_rows < 0";
  if (io.obs_ld < 18) return "obs_ld < 18";
  if (io.out_col < 0 || io.out_ld < (int64_t)io.out_col + 4) return "out_col < 0 or out_ld < out_col + 4";
  if (!io.params || !io.packs || !io.obs || !io.out) return "null params / packs / obs / out";
  if (io.policy && (!io.order || !io.counts || !io.offsets || !tiles_ok)) return "null scratch with policy given";
  return nullptr;
}

extern "C" {

int hkl_act_io_size(void) { return (int)sizeof(hkl_act_io); }
int hkl_act_wide_io_size(void) { return (int)sizeof(hkl_act_wide_io); }

int hkl_act_wide(const hkl_act_wide_io *io, void *stream) {
  const char *who = "hkl_act_wide";
  const auto bad = [](const hkl_act_wide_io &x) { return bad_act(x, HKL_ACT_WIDE_MAX_POLICIES, x.tiles != nullptr); };
  if (const int rc = bad_io(who, io, bad)) return rc;
  if (io->n_rows == 0) return HKL_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = (io->n_rows + 63) / 64;
  if (io->policy) {
    const unsigned rows = blocks(io->n_rows, 256);
    hipLaunchKernelGGL(act_wide_zero_kernel, dim3((unsigned)(io->n_policies / 256 + 1)), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_wide_hist_kernel, dim3(rows), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_wide_scan_kernel, dim3(1), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_wide_scatter_kernel, dim3(rows), dim3(256), 0, st, *io);
    // the non-empty tiles are at most min(n_rows, n_rows / 64 + K); their number is known only on the device
    const int64_t bound = tiles + io->n_policies < io->n_rows ? tiles + io->n_policies : (int64_t)io->n_rows;
    hipLaunchKernelGGL(act_wide_kernel, dim3((unsigned)bound), dim3(WG), 0, st, *io);
  } else {
    hipLaunchKernelGGL(act_wide_kernel, dim3((unsigned)tiles), dim3(WG), 0, st, *io);
  }
  return launched(who);
}

int hkl_act(const hkl_act_io *io, void *stream) {
  const char *who = "hkl_act";
  const auto bad = [](const hkl_act_io &x) { return bad_act(x, HKL_ACT_MAX_POLICIES, true); };
  if (const int rc = bad_io(who, io, bad)) return rc;
  if (io->n_rows == 0) return HKL_OK;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = blocks(io->n_rows, 64);
  if (io->policy) {
    const unsigned rows = blocks(io->n_rows, 256);
    // a memset node here, a kernel in hkl_act_wide (act_wide_zero_kernel's comment): the two stay as they are
    const hipError_t m = hipMemsetAsync(io->counts, 0, sizeof(int32_t) * (HKL_ACT_MAX_POLICIES + 1), st);
    if (m != hipSuccess) return fail(m, who);
    hipLaunchKernelGGL(act_hist_kernel, dim3(rows), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_scan_kernel, dim3(1), dim3(64), 0, st, *io);
    hipLaunchKernelGGL(act_scatter_kernel, dim3(rows), dim3(256), 0, st, *io);
    // sum_k ceil(count_k / 64) <= n_rows / 64 + K tiles, known only on the device: the surplus workgroups return
    hipLaunchKernelGGL(act_kernel, dim3(tiles + (unsigned)io->n_policies), dim3(WG), 0, st, *io);
  } else {
    hipLaunchKernelGGL(act_kernel, dim3(tiles), dim3(WG), 0, st, *io);
  }
  return launched(who);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ C ABI: exploration acting
extern "C" {

int hkl_explore_io_size(void) { return (int)sizeof(hkl_explore_io); }
int hkl_explore_member_size(void) { return (int)sizeof(hkl_explore_member); }

int hkl_explore(const hkl_explore_io *io, const hkl_explore_member *members_host, void *stream) {
  const char *who = "hkl_explore";
  const auto bad = [](const hkl_explore_io &x) { return bad_act(x.act, HKL_ACT_MAX_POLICIES, true); };
  if (const int rc = bad_io(who, io, bad)) return rc;
  const hkl_act_io &act = io->act;
  if (io->rows_per_member <= 0) return invalid(who, "rows_per_member <= 0");
  if (act.n_rows == 0 || act.n_rows % io->rows_per_member) return invalid(who, "n_rows is no positive multiple of rows_per_member");
  const int S = act.n_rows / io->rows_per_member;
  if (const int rc = bad_group(who, members_host, io->members, S)) return rc;
  if (!io->total || !io->calls || !io->count) return invalid(who, "null total / calls / count");
  for (int m = 0; m < S; ++m) {
    const hkl_explore_member &mem = members_host[m];
    if (mem.anneal < HKL_ANNEAL_NONE || mem.anneal > HKL_ANNEAL_EXP) return bad_member(who, m, "anneal id out of range");
    if (mem.noise < HKL_NOISE_NONE || mem.noise > HKL_NOISE_EXTERNAL) return bad_member(who, m, "noise id out of range");
    if (mem.noise == HKL_NOISE_OU && !io->x) return bad_member(who, m, "null x with an OU member");
    if (mem.noise == HKL_NOISE_EXTERNAL && !io->ext) return bad_member(who, m, "null ext with an external member");
  }
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = blocks(act.n_rows, 64);
  if (act.policy) {  // hkl_act's grouping launches as they are, behind a kernel in place of its memset
    const unsigned rows = blocks(act.n_rows, 256);
    hipLaunchKernelGGL(explore_zero_kernel, dim3(1), dim3(128), 0, st, act);
    hipLaunchKernelGGL(act_hist_kernel, dim3(rows), dim3(256), 0, st, act);
    hipLaunchKernelGGL(act_scan_kernel, dim3(1), dim3(64), 0, st, act);
    hipLaunchKernelGGL(act_scatter_kernel, dim3(rows), dim3(256), 0, st, act);
    hipLaunchKernelGGL(explore_kernel, dim3(tiles + (unsigned)act.n_policies), dim3(WG), 0, st, *io);
  } else {
    hipLaunchKernelGGL(explore_kernel, dim3(tiles), dim3(WG), 0, st, *io);
  }
  hipLaunchKernelGGL(explore_advance_kernel, dim3(1), dim3(HKL_GROUP_MAX), 0, st, *io, S);
  return launched(who);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ C ABI: collection
// the member layout both calls share: what is wrong with (n_rows, rows_per_member, pmax), or nullptr
static const char *bad_layout(int32_t n_rows, int32_t n, int32_t pmax) {
  if (n <= 0) return "rows_per_member <= 0";
  if (n_rows <= 0 || n_rows % n) return "n_rows is no positive multiple of rows_per_member";
  if (n_rows / n > HKL_GROUP_MAX) return "n_members (n_rows / rows_per_member) outside [1, HKL_GROUP_MAX]";
  return pmax < 1 ? "pmax < 1" : nullptr;
}
static const char *bad_opp_draw(const hkl_opp_draw_io &io) {
  if (const char *w = bad_layout(io.n_rows, io.rows_per_member, io.pmax)) return w;
  if (!io.seeds || !io.calls || !io.probs || !io.len || !io.scores || !io.slots)
    return "null seeds / calls / probs / len / scores / slots";
  return (!io.policy2 || !io.policy || !io.snap || !io.counts || !io.snap_counts)
             ? "null policy2 / policy / snap / counts / snap_counts" : nullptr;
}
static const char *bad_collect(const hkl_collect_io &io) {
  if (const char *w = bad_layout(io.n_rows, io.rows_per_member, io.pmax)) return w;
  if (io.cap < 1 || io.rows_per_member > io.cap) return "cap < 1 or rows_per_member > cap";
  if (io.act_ld < 4) return "act_ld < 4";
  if (!io.obs || !io.act || !io.obs_next || !io.reward || !io.done) return "null obs / act / obs_next / reward / done";
  if (!io.s || !io.a || !io.r || !io.s2 || !io.d || !io.pos || !io.size) return "null ring column / pos / size";
  if (!io.ep_reward || !io.push_pos || !io.push_n || !io.steps || !io.scratch)
    return "null ep_reward / push_pos / push_n / steps / scratch";
  if (io.snap && !io.tally) return "snap without tally";
  if (io.alive && !io.count) return "alive without count";
  return (io.keep_obs2 && !io.obs2_next) ? "keep_obs2 without obs2_next" : nullptr;
}

extern "C" {

int hkl_opp_draw_io_size(void) { return (int)sizeof(hkl_opp_draw_io); }
int hkl_collect_io_size(void) { return (int)sizeof(hkl_collect_io); }
int64_t hkl_collect_scratch_ints(int32_t n_rows, int32_t rows_per_member) {
  if (rows_per_member <= 0 || n_rows <= 0) return 0;
  return HKL_GROUP_MAX + 3 * (int64_t)(n_rows / rows_per_member) * collect_nb(rows_per_member);
}

int hkl_opp_draw(const hkl_opp_draw_io *io, void *stream) {
  const char *who = "hkl_opp_draw";
  if (const int rc = bad_io(who, io, bad_opp_draw)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int S = io->n_rows / io->rows_per_member;
  hipLaunchKernelGGL(opp_draw_kernel, dim3(blocks(io->rows_per_member, CWG), S), dim3(CWG), 0, st, *io);
  hipLaunchKernelGGL(opp_advance_kernel, dim3(1), dim3(HKL_GROUP_MAX), 0, st, *io, S);
  return launched(who);
}

int hkl_collect(const hkl_collect_io *io, void *stream) {
  const char *who = "hkl_collect";
  if (const int rc = bad_io(who, io, bad_collect)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks(io->rows_per_member, CWG), io->n_rows / io->rows_per_member);
  if (io->alive) {
    hipLaunchKernelGGL(collect_count_kernel, grid, dim3(CWG), 0, st, *io);
    hipLaunchKernelGGL(collect_scan_kernel, dim3(grid.y), dim3(CWG), 0, st, *io);
    hipLaunchKernelGGL(collect_store_kernel<true>, grid, dim3(CWG), 0, st, *io);
  } else {
    hipLaunchKernelGGL(collect_store_kernel<false>, grid, dim3(CWG), 0, st, *io);
  }
  return launched(who);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ C ABI: evaluation
enum EvalCall { kEvalBegin, kEvalStep, kEvalFold };
template <EvalCall K>
static const char *bad_eval(const hkl_eval_io &io) {
  if (io.rows_per_cell <= 0) return "rows_per_cell <= 0";
  if (io.n_rows <= 0 || io.n_rows % io.rows_per_cell) return "n_rows is no positive multiple of rows_per_cell";
  if (io.n_rows / io.rows_per_cell > HKL_EVAL_CELLS_MAX) return "n_cells (n_rows / rows_per_cell) outside [1, HKL_EVAL_CELLS_MAX]";
  if (io.info_ld < 1) return "info_ld < 1";
  if (!io.live || !io.ret || !io.length || !io.winner) return "null live / ret / length / winner";
  if (K == kEvalFold) return (!io.outcomes || !io.length_sum || !io.return_sum) ? "null outcomes / length_sum / return_sum" : nullptr;
  if (!io.seeds || !io.step || !io.count) return "null seeds / step / count";
  return (K == kEvalStep && (!io.reward || !io.done || !io.info)) ? "null reward / done / info" : nullptr;
}

extern "C" {

int hkl_eval_io_size(void) { return (int)sizeof(hkl_eval_io); }

int hkl_eval_begin(const hkl_eval_io *io, void *stream) {
  const char *who = "hkl_eval_begin";
  if (const int rc = bad_io(who, io, bad_eval<kEvalBegin>)) return rc;
  const dim3 grid(blocks(io->rows_per_cell, CWG), io->n_rows / io->rows_per_cell);
  hipLaunchKernelGGL(eval_begin_kernel, grid, dim3(CWG), 0, (hipStream_t)stream, *io);
  return launched(who);
}

int hkl_eval_step(const hkl_eval_io *io, void *stream) {
  const char *who = "hkl_eval_step";
  if (const int rc = bad_io(who, io, bad_eval<kEvalStep>)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks(io->rows_per_cell, CWG), io->n_rows / io->rows_per_cell);
  hipLaunchKernelGGL(eval_step_kernel, grid, dim3(CWG), 0, st, *io);
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(1), 0, st, *io);
  return launched(who);
}

int hkl_eval_fold(const hkl_eval_io *io, void *stream) {
  const char *who = "hkl_eval_fold";
  if (const int rc = bad_io(who, io, bad_eval<kEvalFold>)) return rc;
  hipLaunchKernelGGL(eval_fold_kernel, dim3(io->n_rows / io->rows_per_cell), dim3(CWG), 0, (hipStream_t)stream, *io);
  return launched(who);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ C ABI: twin-critic inference
extern "C" {

int hkl_value_io_size(void) { return (int)sizeof(hkl_value_io); }

int hkl_value(const hkl_value_io *io, void *stream) {  // the only user of hkl_value_io: its checks stand here
  const char *who = "hkl_value";
  if (!io) return invalid(who, "null io");
  if (io->n_rows < 0) return invalid(who, "n_rows < 0");
  if (!io->obs) return invalid(who, "null obs");
  if (io->obs_ld < 18) return invalid(who, "obs_ld < 18");
  if (io->act && io->act_ld < 4) return invalid(who, "act_ld < 4");
  if (io->act && io->act_out) return invalid(who, "act_out is the actor's action: not with act given");
  if (io->act_out && io->act_out_ld < 4) return invalid(who, "act_out_ld < 4");
  if (!io->q1 && !io->q2 && !io->qmin && !io->act_out) return invalid(who, "every output is null");
  if (bad_net(io->q[0]) || bad_net(io->q[1])) return invalid(who, "a critic's weight or pack pointer is null");
  if (!io->act && bad_net(io->actor)) return invalid(who, "the actor's weight or pack pointer is null (act == NULL)");
  if (io->n_rows == 0) return HKL_OK;
  hipLaunchKernelGGL(value_kernel, dim3(blocks(io->n_rows, 64)), dim3(WG), 0, (hipStream_t)stream, *io);
  return launched(who);
}

}  // extern "C"

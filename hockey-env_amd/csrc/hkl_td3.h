// hkl_td3.h -- the TD3 learner's kernels on hkl_mlp.h's layers (hk_learner.hip's head describes the stages): the
// Philox sampler, critic step, actor step, weight gradients, Adam, polyak and pack, each with its *_group twin.
#pragma once
#include "hkl_mlp.h"
#include "hkl_rng.h"  // philox, box_muller

namespace hkl {

// ------------------------------------------------------------------------------------------------ sampling
// The batch's replay slots and target noise from a counter-based RNG (Philox4x32-10 keyed by the learner's seed, the
// counter = (sample, update, purpose)): uniform slots floor(u * size) with a 53-bit u (rl/replay/uniform_buffer.py's
// (rand * size).astype(int)), and the target policy smoothing noise clamp(N(0, scale), -clip, clip) by Box-Muller
// (learner.py:80-93).  The update counter lives in device memory (graph replays advance it): critic_step bumps it.
// sample e's replay slot of update `ctr` over `size` filled slots.  size <= 0 (an empty ring, or a fill word that is
// out of contract) gives slot 0: out-of-contract device values are clamped, never addressed (as per_sample_body)
__device__ __forceinline__ int64_t sample_slot(uint64_t seed, int64_t e, uint64_t ctr, int64_t size) {
  if (size <= 0) return 0;
  const P4 r0 = philox(seed, P4{(uint32_t)e, (uint32_t)(e >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32)});
  const uint64_t bits = (((uint64_t)r0.x << 32) | r0.y) >> 11;
  const double u = (double)bits * (1.0 / 9007199254740992.0);
  const uint64_t i = (uint64_t)(u * (double)(uint64_t)size);
  return (int64_t)(i < (uint64_t)size ? i : (uint64_t)size - 1);
}
// sample e's clipped target-smoothing noise of update `ctr`
__device__ __forceinline__ f4 sample_noise(uint64_t seed, int64_t e, uint64_t ctr, float scale, float clip) {
  float z[4];
  box_muller(philox_at(seed ^ 0x6E6F697365ull, e, ctr), z);
  f4 nz;
#pragma unroll
  for (int c = 0; c < 4; ++c) nz[c] = fminf(fmaxf(z[c] * scale, -clip), clip);
  return nz;
}
// Every learner kernel's body is a __device__ function of its io struct: the single-member kernel passes its by-value
// argument, the grouped twin (the *_group_kernel after it) member m's struct from an array in device memory, m taken
// from a grid dimension the body does not read.  The struct reads are wave-uniform either way.
__device__ __forceinline__ void sample_body(const hkl_sample_io &io) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= io.batch) return;
  const uint64_t ctr = (uint64_t)*io.counter;
  io.idx[e] = sample_slot(io.seed, e, ctr, *io.size);
  *reinterpret_cast<f4 *>(io.noise + e * 4) = sample_noise(io.seed, e, ctr, io.scale, io.clip);
}
__global__ void __launch_bounds__(256) sample_kernel(hkl_sample_io io) { sample_body(io); }
__global__ void __launch_bounds__(256) sample_group_kernel(const hkl_sample_io *__restrict__ ios) {
  sample_body(ios[blockIdx.y]);
}

// ------------------------------------------------------------------------------------------------ critic step
// Q(x) of one critic network (forward only): its output for this lane's sample
__device__ __forceinline__ float q_forward(const Net &c, const float (&x)[S1], Tile &h1, Tile &h2, int lane,
                                           f4 *sfrag) {
  gemm_in(c.f1(), x, h1, lane, sfrag);
  gemm256(c.fp(), h1, c.b1, h2, lane, sfrag);
  return head1(c.w3, h2, c.b2, c.b3, lane);
}

// one critic k of update_critic: forward on x, the weighted smooth-L1 (torch_utils.py:12-24; critic_loss =
// (loss1 + loss2) * 0.5, each a batch mean) and the backward to the first layer.  Stores H1, DZ1, DZ2 for the
// weight gradients (their bias gradients are the column sums wgrad takes); dW3 / db3 as workgroup partials.
__device__ __forceinline__ void critic_one(const hkl_critic_io &io, int k, const Net &c, const float (&x)[S1], float y,
                                           float w, int64_t row, float *red, f4 *sfrag, float &td, float &loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
  Tile h1, h2;
  gemm_in(c.f1(), x, h1, lane, sfrag);
  gemm256(c.fp(), h1, c.b1, h2, lane, sfrag);
  store_tile(io.h1[k], h1, row, q);
  const float qv = head1(c.w3, h2, c.b2, c.b3, lane);
  const float diff = qv - y, ad = fabsf(diff);
  loss += ad < 1.0f ? 0.5f * w * diff * diff : (ad - 0.5f) * w;
  const float g = (ad < 1.0f ? w * diff : (diff > 0.0f ? w : diff < 0.0f ? -w : 0.0f)) * (0.5f / (float)io.batch);
  td += ad;
  // output layer: dW3 = sum_j g_j h2_j, db3 = sum_j g_j
  Tile t;
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) t.v[ob] = h2.v[ob] * g;
  wg_neuron_sum(t, red, io.p_dw3[k] + blockIdx.x * H, wave, lane);
  const float gb = wg_scalar_sum(g, red, wave, lane);
  if (threadIdx.x == 0) io.p_db3[k][blockIdx.x] = gb;
  // dz2 = (W3^T g) * (1 - h2^2)
  back_out(c.w3, 1, f4{g, 0.0f, 0.0f, 0.0f}, t, q);
  tanh_back(t, h2);
  store_tile(io.dz2[k], t, row, q);
  // dz1 = (W2^T dz2) * (1 - h1^2)
  gemm256(c.bp(), t, nullptr, h2, lane, sfrag);
  tanh_back(h2, h1);
  store_tile(io.dz1[k], h2, row, q);
}

// compute_target + update_critic's forward / loss / backward for both critics (learner.py:75-136).
__device__ __forceinline__ void critic_step_body(const hkl_critic_io &io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];  // two fragment buffers + the staged bias
  __shared__ float red[4 * H];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + j;  // this lane's sample (batch row)
  const int64_t src = io.idx[row];                                // its replay slot
  const float *s_row = io.ring_s + src * 18, *s2_row = io.ring_s2 + src * 18;
  const float rwd = io.ring_r[src], dn = io.ring_d[src];
  const f4 act = *reinterpret_cast<const f4 *>(io.ring_a + src * 4);
  const f4 nz = *reinterpret_cast<const f4 *>(io.noise + row * 4);
  const float w = io.iw ? io.iw[row] : 1.0f;
  const Net ta = net_of(io.target_actor), tq[2] = {net_of(io.target_q[0]), net_of(io.target_q[1])};
  const Net cq[2] = {net_of(io.q[0]), net_of(io.q[1])};

  // ---- target: y = r + gamma (1 - d) min(Q1', Q2')(s2, clamp(actor'(s2) + noise, -1, 1))
  float x[S1];
  input_frags(s2_row, z4(), false, x, q);
  Tile h1, h2;
  gemm_in(ta.f1(), x, h1, lane, sfrag);
  gemm256(ta.fp(), h1, ta.b1, h2, lane, sfrag);
  const f4 a2 = gemm_out(ta.fo(), h2, ta.b2, ta.b3, 4, lane, sfrag);
  f4 a2u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float t = fminf(fmaxf(tanh_fast(a2[c]) + nz[c], -1.0f), 1.0f);  // torch.clamp(target_action + noise, -1, 1)
    a2u[c] = unscale(t, io.act_low[c], io.act_range[c]);
  }
  input_frags(s2_row, a2u, true, x, q);
  const float qt0 = q_forward(tq[0], x, h1, h2, lane, sfrag), qt1 = q_forward(tq[1], x, h1, h2, lane, sfrag);
  const float y = rwd + io.gamma * (1.0f - dn) * fminf(qt0, qt1);

  // ---- critics on (s, a)
  f4 au;
#pragma unroll
  for (int c = 0; c < 4; ++c) au[c] = unscale(act[c], io.act_low[c], io.act_range[c]);
  input_frags(s_row, au, true, x, q);
  {  // X0 row (shared by both critics' dW1): 22 features, zero padded; lane q writes 8 of its sample's 32
    float *xr = io.x0 + row * XP;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int f = 8 * q + e;
      xr[f] = f < 18 ? s_row[f] : f < 22 ? au[f - 18] : 0.0f;
    }
  }
  float td = 0.0f, loss = 0.0f;
  critic_one(io, 0, cq[0], x, y, w, row, red, sfrag, td, loss);
  critic_one(io, 1, cq[1], x, y, w, row, red, sfrag, td, loss);
  if (io.td && q == 0) io.td[row] = td * 0.5f;  // (|q1 - y| + |q2 - y|) / 2 (learner.py:163-170)
  const float ls = wg_scalar_sum(loss, red, wave, lane);
  if (threadIdx.x == 0) io.p_loss[blockIdx.x] = ls;
  if (io.sample_counter && blockIdx.x == 0 && threadIdx.x == 0) *io.sample_counter += 1;
}
__global__ void __launch_bounds__(WG, 1) critic_step_kernel(hkl_critic_io io) { critic_step_body(io); }
__global__ void __launch_bounds__(WG, 1) critic_step_group_kernel(const hkl_critic_io *__restrict__ ios) {
  critic_step_body(ios[blockIdx.y]);
}

// ------------------------------------------------------------------------------------------------ actor step
// update_actor's forward / backward (learner.py:138-175): loss = -mean Q1(s, actor(s)) with the updated critic.
__device__ __forceinline__ void actor_step_body(const hkl_actor_io &io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];  // two fragment buffers + the staged bias
  __shared__ float red[4 * H];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + j;
  const int64_t src = io.idx[row];
  const float *s_row = io.ring_s + src * 18;
  const Net an = net_of(io.actor), qn = net_of(io.q1);
  float x[S1];
  input_frags(s_row, z4(), false, x, q);
  {
    float *xr = io.x0 + row * XP;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int f = 8 * q + e;
      xr[f] = f < 18 ? s_row[f] : 0.0f;
    }
  }
  Tile h1, h2;
  gemm_in(an.f1(), x, h1, lane, sfrag);
  gemm256(an.fp(), h1, an.b1, h2, lane, sfrag);
  store_tile(io.h1, h1, row, q);
  const f4 pre = gemm_out(an.fo(), h2, an.b2, an.b3, 4, lane, sfrag);
  store_tile(io.h2, h2, row, q);
  f4 a, au;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    a[c] = tanh_fast(pre[c]);
    au[c] = unscale(a[c], io.act_low[c], io.act_range[c]);
  }
  // Q1(s, a)
  input_frags(s_row, au, true, x, q);
  gemm_in(qn.f1(), x, h1, lane, sfrag);
  gemm256(qn.fp(), h1, qn.b1, h2, lane, sfrag);
  const float qv = gemm_out(qn.fo(), h2, qn.b2, qn.b3, 1, lane, sfrag)[0];
  const float g = -1.0f / (float)io.batch;  // d(-mean q) / dq
  Tile t;
  back_out(qn.w3, 1, f4{g, 0.0f, 0.0f, 0.0f}, t, q);
  tanh_back(t, h2);
  gemm256(qn.bp(), t, nullptr, h2, lane, sfrag);
  tanh_back(h2, h1);  // dz1 of Q1
  // dQ/d(unscaled action) = W1[:, 18:22]^T dz1, summed over the 4 lanes of the sample; then the unscale chain rule
  f4 da = z4();
  const f4 *wa = qn.wa();
#pragma unroll
  for (int ob = 0; ob < 16; ++ob)
#pragma unroll
    for (int r = 0; r < 4; ++r) da += wa[16 * ob + 4 * q + r] * h2.v[ob][r];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float v = da[c];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    da[c] = v * (2.0f / io.act_range[c]);
  }
  // actor output layer: dz3 = da * (1 - a^2); dW3 = sum_j dz3_j h2_j; db3 = sum_j dz3_j
  f4 dz3;
#pragma unroll
  for (int c = 0; c < 4; ++c) dz3[c] = da[c] * (1.0f - a[c] * a[c]);
  load_tile(io.h2, h2, row, q);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int ob = 0; ob < 16; ++ob) t.v[ob] = h2.v[ob] * dz3[c];
    wg_neuron_sum(t, red, io.p_dw3 + ((int64_t)blockIdx.x * 4 + c) * H, wave, lane);
    const float gb = wg_scalar_sum(dz3[c], red, wave, lane);
    if (threadIdx.x == 0) io.p_db3[blockIdx.x * 4 + c] = gb;
  }
  back_out(an.w3, 4, dz3, t, q);
  tanh_back(t, h2);
  store_tile(io.dz2, t, row, q);
  gemm256(an.bp(), t, nullptr, h2, lane, sfrag);
  load_tile(io.h1, h1, row, q);
  tanh_back(h2, h1);
  store_tile(io.dz1, h2, row, q);
  const float ls = wg_scalar_sum(-qv, red, wave, lane);
  if (threadIdx.x == 0) io.p_loss[blockIdx.x] = ls;
}
__global__ void __launch_bounds__(WG, 1) actor_step_kernel(hkl_actor_io io) { actor_step_body(io); }
__global__ void __launch_bounds__(WG, 1) actor_step_group_kernel(const hkl_actor_io *__restrict__ ios) {
  actor_step_body(ios[blockIdx.y]);
}

// ------------------------------------------------------------------------------------------------ weight gradients
// dW[o][k] = sum_j DZ[j][o] X[j][k] over one chunk of CHUNK samples, o in 128-row tiles, k in KT-wide tiles; 4 waves
// as 2 (o) x 2 (k).  The chunk streams through two LDS buffers 32 samples at a time (the next sub-chunk's loads are
// in flight while the current one is multiplied).  Output: slab[chunk][256][ldx] (natural W layout, fp32 partial
// sums; the adam kernel adds the chunks in order).  Blocks of the first k tile also sum DZ's columns: the bias
// gradient partials bslab[chunk][256].  One launch runs up to 4 jobs (blockIdx.z = job * chunks + chunk).
struct WgJob {
  const float *dz, *x;
  float *slab, *bslab;
  int ldx;
};
struct WgJobs {
  WgJob job[4];
  int chunks, chunk_size;
};
constexpr int kWgSub = 32, kWgOt = 128, kWgPad = 4;
// One split-K tile of dW = DZ^T X: output rows [o0, o0 + 128) x k columns [k0, k0 + KT) of one job, summed over chunk
// `chunk` of csize samples (sa / sb: this block's double-buffered LDS staging, [2][32][128 + 4] and [2][32][KT + 4]).
template <int KT>
__device__ __forceinline__ void wgrad_tile(const WgJob &job, int bx, int by, int chunk, int csize,
                                           float (*sa)[kWgSub][kWgOt + kWgPad], float (*sb)[kWgSub][KT + kWgPad]) {
  constexpr int SUB = kWgSub, OT = kWgOt;
  constexpr int NB = KT == 128 ? 4 : 1;  // 16-column blocks per wave
  constexpr int LA = SUB * OT / 4 / WG, LB = (SUB * KT / 4 + WG - 1) / WG;  // f4 loads per thread per sub-chunk
  const float *__restrict__ dz = job.dz;
  const float *__restrict__ xs = job.x;
  float *__restrict__ slab = job.slab;
  float *__restrict__ bslab = job.bslab;
  const int ldx = job.ldx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kk = lane >> 4, i = lane & 15;
  const int wo = wave >> 1, wk = wave & 1;
  const int o0 = bx * OT, k0 = by * KT;
  const int64_t j0 = (int64_t)chunk * csize;
  const bool bias = bslab != nullptr && by == 0;
  f4 acc[4][NB];
#pragma unroll
  for (int bo = 0; bo < 4; ++bo)
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) acc[bo][bk] = z4();
  float bsum = 0.0f;  // thread t < OT: column o0 + t of DZ
  f4 ga[LA], gb[LB];
  auto fetch = [&](int sub) {
#pragma unroll
    for (int u = 0; u < LA; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (OT / 4), cc = (e % (OT / 4)) * 4;
      ga[u] = *reinterpret_cast<const f4 *>(dz + (j0 + sub + rr) * H + o0 + cc);
    }
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (KT / 4), cc = (e % (KT / 4)) * 4;
      if (e < SUB * KT / 4) gb[u] = *reinterpret_cast<const f4 *>(xs + (j0 + sub + rr) * ldx + k0 + cc);
    }
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int u = 0; u < LA; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (OT / 4), cc = (e % (OT / 4)) * 4;
      *reinterpret_cast<f4 *>(&sa[b][rr][cc]) = ga[u];
    }
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (KT / 4), cc = (e % (KT / 4)) * 4;
      if (e < SUB * KT / 4) *reinterpret_cast<f4 *>(&sb[b][rr][cc]) = gb[u];
    }
  };
  fetch(0);
  for (int sub = 0, b = 0; sub < csize; sub += SUB, b ^= 1) {
    stash(b);
    __syncthreads();
    if (sub + SUB < csize) fetch(sub + SUB);
    if (bias && threadIdx.x < OT) {
      // the sub-chunk's 32 rows as four interleaved partial sums joined as a tree, then added to the chunk's sum:
      // one running sum over the chunk's 256 or 512 signed terms lost a few ulp more than torch's blocked column
      // sum does (tests/test_gpu_learner_kernels.py measures both against float64)
      float ps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < SUB; ++r) ps[r & 3] += sa[b][r][threadIdx.x];
      bsum += (ps[0] + ps[1]) + (ps[2] + ps[3]);
    }
#pragma unroll
    for (int s = 0; s < SUB / 4; ++s) {
      const f4 A = *reinterpret_cast<const f4 *>(&sa[b][4 * s + kk][64 * wo + 4 * i]);  // rows o = 64 wo + 4 i + bo
      f4 B;
      if constexpr (NB == 4) B = *reinterpret_cast<const f4 *>(&sb[b][4 * s + kk][64 * wk + 4 * i]);  // k = 64 wk + 4 i + bk
      else B[0] = sb[b][4 * s + kk][16 * wk + i];                                                // k = 16 wk + i
#pragma unroll
      for (int bo = 0; bo < 4; ++bo)
#pragma unroll
        for (int bk = 0; bk < NB; ++bk) acc[bo][bk] = mfma(A[bo], B[bk], acc[bo][bk]);
    }
  }
  if (bias && threadIdx.x < OT) bslab[(int64_t)chunk * H + o0 + threadIdx.x] = bsum;
  // acc[bo][bk] lane (jj = i, q = kk) reg r: o = o0 + 64 wo + 4 (4 q + r) + bo, k = k0 + (NB == 4 ? 64 wk + 4 jj + bk : 16 wk + jj)
  float *dst = slab + (int64_t)chunk * H * ldx;
#pragma unroll
  for (int bo = 0; bo < 4; ++bo)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = o0 + 64 * wo + 4 * (4 * kk + r) + bo;
      if constexpr (NB == 4) {
        const f4 v = f4{acc[bo][0][r], acc[bo][1][r], acc[bo][2][r], acc[bo][3][r]};
        *reinterpret_cast<f4 *>(dst + (int64_t)o * ldx + k0 + 64 * wk + 4 * i) = v;
      } else {
        dst[(int64_t)o * ldx + k0 + 16 * wk + i] = acc[bo][0][r];
      }
    }
}

template <int KT>
__global__ void __launch_bounds__(WG, 1) wgrad_kernel(WgJobs jobs) {
  __shared__ float sa[2][kWgSub][kWgOt + kWgPad];
  __shared__ float sb[2][kWgSub][KT + kWgPad];
  const int bz = blockIdx.z;
  wgrad_tile<KT>(jobs.job[bz / jobs.chunks], blockIdx.x, blockIdx.y, bz % jobs.chunks, jobs.chunk_size, sa, sb);
}

// hkl_wgrad_pair: a network's dW2 tiles (k width 256) and dW1 tiles (k width 32) in one launch -- blocks
// [0, n_wide) take the wide jobs (grid 2 x 2 x chunks per job), the rest the narrow ones (2 x 1 x chunks), so the
// short dW1 tiles fill the SIMDs the dW2 tiles leave and one launch gap is saved.  The narrow tile's staging
// lives inside the wide one's (same LDS as a wide-only block).
// One block of the pair: jobs are read through job_of(width, j), which the single kernel answers from its by-value
// WgJobs and the grouped one from member blockIdx.y's hkl_wgrad_job rows in device memory.
template <class JobOf>
__device__ __forceinline__ void wgrad_pair_body(const JobOf &job_of, int chunks_wide, int csize_wide, int chunks_narrow,
                                                int csize_narrow, int n_wide) {
  __shared__ float sa[2][kWgSub][kWgOt + kWgPad];
  __shared__ float sb[2][kWgSub][128 + kWgPad];
  static_assert(sizeof(float[2][kWgSub][XP + kWgPad]) <= sizeof(sb), "the narrow staging fits the wide one");
  const int id = blockIdx.x;
  if (id < n_wide) {
    const int z = id >> 2;
    wgrad_tile<128>(job_of(true, z / chunks_wide), id & 1, (id >> 1) & 1, z % chunks_wide, csize_wide, sa, sb);
  } else {
    const int j = id - n_wide, z = j >> 1;
    wgrad_tile<XP>(job_of(false, z / chunks_narrow), j & 1, 0, z % chunks_narrow, csize_narrow, sa,
                   reinterpret_cast<float(*)[kWgSub][XP + kWgPad]>(&sb[0][0][0]));
  }
}
__global__ void __launch_bounds__(WG, 1) wgrad_pair_kernel(WgJobs wide, WgJobs narrow, int n_wide) {
  wgrad_pair_body([&](bool w, int j) -> const WgJob & { return w ? wide.job[j] : narrow.job[j]; }, wide.chunks,
                  wide.chunk_size, narrow.chunks, narrow.chunk_size, n_wide);
}
// member blockIdx.y's jobs: rows [m * n_jobs, (m + 1) * n_jobs) of the two device arrays
struct WgGroup {
  const hkl_wgrad_job *wide, *narrow;
  int n_wide_jobs, n_narrow_jobs;
  int chunks_wide, csize_wide, chunks_narrow, csize_narrow;
  int n_wide;  // wide blocks per member
};
__global__ void __launch_bounds__(WG, 1) wgrad_pair_group_kernel(WgGroup g) {
  const int m = blockIdx.y;
  wgrad_pair_body(
      [&](bool w, int j) {
        const hkl_wgrad_job &d = w ? g.wide[m * g.n_wide_jobs + j] : g.narrow[m * g.n_narrow_jobs + j];
        return WgJob{d.dz, d.x, d.slab, d.bias_slab, w ? 256 : XP};
      },
      g.chunks_wide, g.csize_wide, g.chunks_narrow, g.csize_narrow, g.n_wide);
}

// ------------------------------------------------------------------------------------------------ Adam
// grad(e) = sum over chunks c (in order) of src[c * stride + row(e) * ld + col(e)]; then torch.optim.Adam (L2 weight
// decay, bias-corrected moments).  step: the optimiser's step count before this update (device, advanced by pack).
__device__ __forceinline__ void adam_body(const hkl_adam_io &io) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int sidx = -1;
  int64_t base = 0;
  for (int s = 0; s < io.n_seg; ++s) {
    const int64_t n = (int64_t)io.seg[s].rows * io.seg[s].cols;
    if (e < base + n) {
      sidx = s;
      break;
    }
    base += n;
  }
  if (sidx >= 0) {
    const hkl_seg &S = io.seg[sidx];
    const int64_t k = e - base;
    const int64_t rr = k / S.cols, cc = k % S.cols;
    const float *src = S.src + rr * S.ld + cc;
    // 16 partial sums (chunk c into p16[c & 15], in increasing c), summed in a fixed tree; up to 64 slab loads in
    // flight per thread (the reduction is bound by memory-level parallelism: ~2 workgroups per CU at the C5
    // parameter counts)
    float p16[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) p16[u] = 0.0f;
    int c = 0;
    for (; c + 64 <= S.chunks; c += 64) {  // four rounds' loads in flight at once, added in the same order
      float q[64];
#pragma unroll
      for (int u = 0; u < 64; ++u) q[u] = src[(int64_t)(c + u) * S.stride];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 16; ++u) p16[u] += q[16 * r + u];
    }
    for (; c + 32 <= S.chunks; c += 32) {  // two rounds' loads in flight at once, added in the same order
      float q[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) q[u] = src[(int64_t)(c + u) * S.stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) p16[u] += q[u];
#pragma unroll
      for (int u = 0; u < 16; ++u) p16[u] += q[16 + u];
    }
    for (; c + 16 <= S.chunks; c += 16) {
      float q[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) q[u] = src[(int64_t)(c + u) * S.stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) p16[u] += q[u];
    }
    for (; c < S.chunks; ++c) p16[c & 15] += src[(int64_t)c * S.stride];
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
      for (int u = 0; u < h; ++u) p16[u] = p16[u] + p16[u + h];
    float g = p16[0];
    float p = S.param[k];
    if (io.wd != 0.0f) g += io.wd * p;
    const float t = (float)(*io.step + 1);
    float m = S.m[k], v = S.v[k];
    // 1 - beta is taken in double and then rounded, as torch rounds its Python scalar: 1.0f - 0.999f is 1.3e-5 off
    // 0.001 (and 1.0f - 0.9f 2.4e-7 off 0.1), a scale error on every v (m) that no summation order accounts for
    const float beta1 = (float)io.beta1, beta2 = (float)io.beta2;
    const float omb1 = (float)(1.0 - io.beta1), omb2 = (float)(1.0 - io.beta2);
    m = m + (g - m) * omb1;  // exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + omb2 * g * g;
    const float bc1 = 1.0f - powf(beta1, t), bc2 = 1.0f - powf(beta2, t);
    const float denom = sqrtf(v) / sqrtf(bc2) + io.eps;
    p = p - (io.lr / bc1) * (m / denom);
    S.m[k] = m;
    S.v[k] = v;
    S.param[k] = p;
    if (io.polyak && S.target)  // soft_update with the new parameter: target.mul_(rho).add_(tau * param)
      S.target[k] = __fadd_rn(__fmul_rn(S.target[k], io.polyak_rho), __fmul_rn(io.polyak_tau, p));
  }
  if (blockIdx.x == 0 && io.loss_src) {
    // the step's loss: the sum of the workgroup partials (scaled), into the learner's accumulator -- a fixed-order
    // tree over workgroup 0's 256 threads (one thread summing 256 dependent loads was this kernel's tail)
    __shared__ float lred[256];
    float s = 0.0f;
    for (int c = threadIdx.x; c < io.loss_chunks; c += 256) s += io.loss_src[c];
    lred[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
      if ((int)threadIdx.x < h) lred[threadIdx.x] = lred[threadIdx.x] + lred[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      *io.loss_sum += (double)(lred[0] * io.loss_scale);
      *io.loss_count += 1.0;
    }
  }
}
__global__ void __launch_bounds__(256) adam_kernel(hkl_adam_io io) { adam_body(io); }
__global__ void __launch_bounds__(256) adam_group_kernel(const hkl_adam_io *__restrict__ ios) {
  adam_body(ios[blockIdx.y]);
}

// target <- target * rho + tau * param (learner.py:214-218: mul_(rho), add_((1 - rho) * param); tau = 1 - rho
// rounded to fp32 like the reference's scalar)
__global__ void __launch_bounds__(256) polyak_kernel(float *__restrict__ t, const float *__restrict__ p, int64_t n, float rho,
                                                     float tau) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) t[e] = t[e] * rho + tau * p[e];
}

__global__ void tanh_probe_kernel(const float *x, float *y, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) y[e] = tanh_fast(x[e]);
}

// ------------------------------------------------------------------------------------------------ packing
__device__ __forceinline__ void pack_body(const hkl_pack_io &io) {
  const hkl_net &N = io.net[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.y == 0 && e == 0 && io.step) *io.step += 1;  // the optimiser step this pack follows
  if (e >= kPackFloats) return;
  float *pk = N.pack;
  float v = 0.0f;
  if (e < kF1) {
    const int ob = (int)(e / 512), l = (int)(e / 8 % 64), s = (int)(e % 8);
    const int o = 16 * ob + (l & 15), c = 4 * s + (l >> 4);
    v = (s < S1 && c < N.n_in) ? N.w1[o * N.n_in + c] : 0.0f;
  } else if (e < kF1 + kFp) {
    const int64_t k = e - kF1;
    const int ob = (int)(k / 4096), kb = (int)(k / 256 % 16), l = (int)(k / 4 % 64), r = (int)(k % 4);
    v = N.w2[(16 * ob + (l & 15)) * H + 16 * kb + 4 * (l >> 4) + r];
  } else if (e < kF1 + kFp + kBp) {
    const int64_t k = e - kF1 - kFp;
    const int ib = (int)(k / 4096), ob = (int)(k / 256 % 16), l = (int)(k / 4 % 64), r = (int)(k % 4);
    v = N.w2[(16 * ob + 4 * (l >> 4) + r) * H + 16 * ib + (l & 15)];
  } else if (e < kF1 + kFp + kBp + kFo) {
    const int64_t k = e - kF1 - kFp - kBp;
    const int kb = (int)(k / 256), l = (int)(k / 4 % 64), r = (int)(k % 4);
    const int o = l & 15;
    v = o < N.n_out ? N.w3[o * H + 16 * kb + 4 * (l >> 4) + r] : 0.0f;
  } else {
    const int64_t k = e - kF1 - kFp - kBp - kFo;
    const int n = (int)(k / 4), c = (int)(k % 4);
    v = N.n_in == 22 ? N.w1[n * 22 + 18 + c] : 0.0f;
  }
  pk[e] = v;
}
__global__ void __launch_bounds__(256) pack_kernel(hkl_pack_io io) { pack_body(io); }
__global__ void __launch_bounds__(256) pack_group_kernel(const hkl_pack_io *__restrict__ ios) {
  pack_body(ios[blockIdx.z]);
}

}  // namespace hkl
